// genesteps_host.cpp -- the part of the gene homoplasy test (include/peprml.h) that needs no device: the option checks, every gene's
// domain and the -1 rule, the draws (genesteps.hpp, the functions k_steps_resample runs), the per-gene totals and the order
// statistic.  Plain C++: no HIP include, so it builds and runs alone (tests/genesteps_standalone).
#include <algorithm>
#include <cmath>

#include "../../include/peprml.h"
#include "genesteps.hpp"

namespace pml {

int gs_plan(const GsOpts &o, int ngenes, const long long *col_start, int only, GsPlan &plan, std::string &err) {
    if (ngenes < 1 || !col_start) { err = "no genes"; return PML_EINVAL; }
    if (o.statistic < PML_STEPS_RAW || o.statistic > PML_STEPS_MIN_RATIO) { err = "statistic must be PML_STEPS_RAW, PML_STEPS_BEYOND_MIN or PML_STEPS_MIN_RATIO"; return PML_EINVAL; }
    if (o.reps < 1 || o.multiple < 0) { err = "reps must be positive and multiple must not be negative"; return PML_EINVAL; }
    if (col_start[0] != 0) { err = "col_start must begin at 0"; return PML_EINVAL; }
    for (int g = 0; g < ngenes; ++g) if (col_start[g + 1] < col_start[g]) { err = "col_start must not decrease"; return PML_EINVAL; }
    if (col_start[ngenes] >= (1ll << 31)) { err = "the concatenation has 2^31 columns or more"; return PML_EINVAL; }
    if ((long long)ngenes * o.reps >= (1ll << 31)) { err = "ngenes * reps is 2^31 or more"; return PML_EINVAL; }
    const double kd = std::ceil((double)o.reps * o.alpha);
    if (!(kd >= 1.0 && kd <= (double)o.reps)) { err = "ceil(reps * alpha) must lie in [1, reps] (the reference indexes out of bounds)"; return PML_EINVAL; }
    plan.k = (int)kd;
    plan.table_cols.clear();
    plan.split.assign((size_t)ngenes, 0); plan.len.assign((size_t)ngenes, 0); plan.U.assign((size_t)ngenes, 0); plan.run.assign((size_t)ngenes, 1);
    for (int g = 0; g < ngenes; ++g) {
        plan.len[(size_t)g] = (uint32_t)(col_start[g + 1] - col_start[g]);
        if (o.mask && o.mask[g]) continue;
        plan.split[(size_t)g] = (uint32_t)plan.table_cols.size();
        for (long long c = col_start[g]; c < col_start[g + 1]; ++c) plan.table_cols.push_back(c);
    }
    const uint32_t total = (uint32_t)plan.table_cols.size();
    for (int g = 0; g < ngenes; ++g) {
        const bool masked = o.mask && o.mask[g];
        const uint32_t len = plan.len[(size_t)g], U = masked ? total : total - len;
        plan.U[(size_t)g] = U;
        if (masked) plan.split[(size_t)g] = U;
        if (o.multiple > 0 && (unsigned long long)U < (unsigned long long)len * (unsigned)o.multiple) { plan.run[(size_t)g] = 0; continue; }
        if (only >= 0 && g != only) continue;                  // a door for one gene answers for that gene
        if (!o.replace && U < len) {
            err = "gene " + std::to_string(g) + " has " + std::to_string(len) + " columns and only " + std::to_string(U) +
                  " others to draw from without replacement (the reference loops for ever)";
            return PML_EINVAL;
        }
        if (o.replace && U == 0 && len > 0) { err = "gene " + std::to_string(g) + " has no column to draw from (the reference throws)"; return PML_EINVAL; }
    }
    return PML_OK;
}

void gs_draw_columns(const GsOpts &o, const GsPlan &plan, int gene, int rep, long long *cols_out) {
    const uint32_t len = plan.len[(size_t)gene], U = plan.U[(size_t)gene], split = plan.split[(size_t)gene];
    const uint64_t key = gs_key(gs_base(o.seed), gene, o.reps, rep);
    const uint64_t K = gs_mix64(key);
    const int h = gs_half_bits(U);
    for (uint32_t j = 0; j < len; ++j) {
        const uint32_t u = o.replace ? gs_draw(key, j, U) : gs_perm(K, U, h, j);
        cols_out[j] = plan.table_cols[gs_table_index(u, split, len)];
    }
}

void gs_totals(int ngenes, const long long *col_start, const int *steps, const int *min_steps, long long *gene_steps, long long *gene_beyond, float *gene_ratio) {
    for (int g = 0; g < ngenes; ++g) {
        long long s = 0, b = 0; float r = 0;
        for (long long c = col_start[g]; c < col_start[g + 1]; ++c) {
            s += steps[c]; b += steps[c] - min_steps[c];
            const float q = (float)steps[c] / (float)(min_steps[c] + 1);
            if (q == q) r += q;                                    // :97, the Java skips NaN
        }
        gene_steps[g] = s; gene_beyond[g] = b; gene_ratio[g] = r;
    }
}

double gs_order_statistic(double *sums, int reps, int k, double observed, long long *n_ge) {
    std::sort(sums, sums + reps);
    if (n_ge) *n_ge = (long long)(sums + reps - std::lower_bound(sums, sums + reps, observed));
    return sums[reps - k];
}

}  // namespace pml

extern "C" int pml_step_draws_host(const pml_step_threshold_opts *opts, int ngenes, const long long *col_start, int gene, int rep, long long *cols_out) {
    if (!opts || !col_start || !cols_out || ngenes < 1 || gene < 0 || gene >= ngenes || rep < 0 || rep >= opts->reps) return PML_EINVAL;
    try {
        const pml::GsOpts o{opts->statistic, opts->replace, opts->multiple, opts->reps, opts->alpha, opts->seed, opts->mask};
        pml::GsPlan plan; std::string err;
        if (int rc = pml::gs_plan(o, ngenes, col_start, gene, plan, err)) return rc;
        if (!plan.run[(size_t)gene]) return PML_EINVAL;
        pml::gs_draw_columns(o, plan, gene, rep, cols_out);
    } catch (const std::exception &) { return PML_ENOMEM; }
    return PML_OK;
}
