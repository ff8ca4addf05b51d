// A program of its own around genesteps_host.cpp (plain C++, no HIP): built under AddressSanitizer and UndefinedBehaviorSanitizer
// by tests/test_genesteps_host.py.  Reads one case from a text file and prints the per-gene totals, every gene's domain, the
// columns every replicate draws, the replicate sums formed from them and the order statistic.
//   line 1: G   line 2: col_start[G + 1]   line 3: steps[ncols]   line 4: min_steps[ncols]
//   line 5: statistic replace multiple reps alpha seed   line 6: G mask values, or a single -1 for no mask
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>

#include "../../include/peprml.h"
#include "../../pepr_amd/csrc/genesteps.hpp"

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    std::ifstream in(argv[1]);
    int G; in >> G;
    std::vector<long long> cs((size_t)G + 1);
    for (auto &v : cs) in >> v;
    const size_t n = (size_t)cs[(size_t)G];
    std::vector<int> steps(n), mins(n);
    for (auto &v : steps) in >> v;
    for (auto &v : mins) in >> v;
    pml_step_threshold_opts o; std::memset(&o, 0, sizeof o);
    in >> o.statistic >> o.replace >> o.multiple >> o.reps >> o.alpha >> o.seed;
    std::vector<unsigned char> mask;
    int first; in >> first;
    if (first >= 0) { mask.assign((size_t)G, 0); mask[0] = (unsigned char)first; for (int g = 1; g < G; ++g) { int v; in >> v; mask[(size_t)g] = (unsigned char)v; } o.mask = mask.data(); }
    if (!in) return 3;

    std::vector<long long> gs((size_t)G), gb((size_t)G); std::vector<float> gr((size_t)G);
    pml::gs_totals(G, cs.data(), steps.data(), mins.data(), gs.data(), gb.data(), gr.data());
    for (int g = 0; g < G; ++g) { unsigned bits; std::memcpy(&bits, &gr[(size_t)g], 4); std::printf("totals %d %lld %lld %08x\n", g, gs[(size_t)g], gb[(size_t)g], bits); }

    const pml::GsOpts po{o.statistic, o.replace, o.multiple, o.reps, o.alpha, o.seed, o.mask};
    pml::GsPlan plan; std::string err;
    const int rc = pml::gs_plan(po, G, cs.data(), -1, plan, err);
    if (rc) { std::printf("plan error %d %s\n", rc, err.c_str()); return 0; }
    std::printf("k %d\n", plan.k);
    for (int g = 0; g < G; ++g) {
        std::printf("plan %d run %d U %u\n", g, (int)plan.run[(size_t)g], plan.U[(size_t)g]);
        const size_t len = (size_t)(cs[(size_t)g + 1] - cs[(size_t)g]);
        std::vector<long long> cols(len + 1), again(len + 1);
        if (!plan.run[(size_t)g]) {
            if (pml_step_draws_host(&o, G, cs.data(), g, 0, cols.data()) != PML_EINVAL) return 4;
            continue;
        }
        std::vector<double> sums((size_t)o.reps);
        for (int b = 0; b < o.reps; ++b) {
            pml::gs_draw_columns(po, plan, g, b, cols.data());
            if (pml_step_draws_host(&o, G, cs.data(), g, b, again.data()) != PML_OK) return 5;
            if (std::memcmp(cols.data(), again.data(), len * sizeof(long long)) != 0) return 6;
            std::printf("draw %d %d", g, b);
            int isum = 0; float fsum = 0;
            for (size_t j = 0; j < len; ++j) {
                const long long c = cols[j];
                std::printf(" %lld", c);
                if (o.statistic == PML_STEPS_MIN_RATIO) fsum += (float)steps[(size_t)c] / (float)(mins[(size_t)c] + 1);
                else isum += o.statistic == PML_STEPS_RAW ? steps[(size_t)c] : steps[(size_t)c] - mins[(size_t)c];
            }
            std::printf("\n");
            sums[(size_t)b] = o.statistic == PML_STEPS_MIN_RATIO ? (double)fsum : (double)isum;
        }
        const double observed = o.statistic == PML_STEPS_RAW ? (double)gs[(size_t)g] : o.statistic == PML_STEPS_BEYOND_MIN ? (double)gb[(size_t)g] : (double)gr[(size_t)g];
        long long n_ge = 0;
        const double t = pml::gs_order_statistic(sums.data(), o.reps, plan.k, observed, &n_ge);
        std::printf("stat %d %a %lld\n", g, t, n_ge);
    }
    return 0;
}
