// congruence_host.cpp -- the two host rules of the congruence filter (include/peprml.h): which splits are kept, which genes are
// kept.  Plain C++ without HIP: the library links it, and it builds alone with a small main under the host sanitizers.
#include "congruence.hpp"

#include <algorithm>

#include "../../include/peprml.h"

namespace pml {

int cg_kept_set(const int *count, size_t ndistinct, long long top_n, std::vector<size_t> &kept) {
    kept.clear();
    int max = 0; bool any = false;
    for (size_t i = 0; i < ndistinct; ++i) if (count[i] > 0) { any = true; max = std::max(max, count[i]); }
    if (!any) return 0;
    std::vector<long long> dist((size_t)max + 1, 0);           // StatisticsUtilities.getDistribution: dist[c], c in 0..max
    for (size_t i = 0; i < ndistinct; ++i) if (count[i] > 0) dist[(size_t)count[i]]++;
    int cutoff = 0; long long included = 0;
    for (int i = max; i >= 0 && included < top_n; --i) { cutoff = i; included += dist[(size_t)i]; }
    for (size_t i = 0; i < ndistinct; ++i) if (count[i] > 0 && count[i] >= cutoff) kept.push_back(i);
    return cutoff;
}

int cg_select(int ngenes, const long long *mean_cost, double p, int *keep, int *idx_out, long long *max_cost_out) {
    if (ngenes <= 0 || !mean_cost || !keep || !(p > 0)) return -1;        // NaN fails the comparison
    if (p >= 1.0) p /= 100;
    const double at = (double)ngenes - ((double)ngenes * p);
    if (!(at > -1.0) || at >= (double)ngenes) return -1;                  // (int) truncates towards zero; outside the array the Java throws
    const int idx = (int)at;
    std::vector<long long> sorted(mean_cost, mean_cost + ngenes);
    std::sort(sorted.begin(), sorted.end());
    const long long max_cost = sorted[(size_t)idx];
    for (int g = 0; g < ngenes; ++g) keep[g] = g <= idx && mean_cost[g] <= max_cost;
    if (idx_out) *idx_out = idx;
    if (max_cost_out) *max_cost_out = max_cost;
    return 0;
}

}  // namespace pml

extern "C" int pml_congruence_select(int ngenes, const long long *mean_cost, double trim_percent, int *keep_out, int *idx_out, long long *max_cost_out) {
    try {
        return pml::cg_select(ngenes, mean_cost, trim_percent, keep_out, idx_out, max_cost_out) ? PML_EINVAL : PML_OK;
    } catch (...) { return PML_ENOMEM; }
}
