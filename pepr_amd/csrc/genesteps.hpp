// genesteps.hpp -- the draw rules of the gene homoplasy test (include/peprml.h, pml_step_thresholds) as ONE set of functions,
// compiled for the device (k_steps_resample, genesteps.hip) and for the host (pml_step_draws_host, genesteps_host.cpp): the two
// cannot disagree.  Plain C++ outside hipcc; no HIP include.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#if defined(__HIPCC__)
#define PML_GS_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define PML_GS_HD inline
#endif

namespace pml {

// the project's counter hash (kernels.h mix64: splitmix64's finaliser), here for both sides
PML_GS_HD uint64_t gs_mix64(uint64_t z) {
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull; z ^= z >> 27; z *= 0x94D049BB133111EBull; z ^= z >> 31;
    return z;
}
PML_GS_HD uint64_t gs_base(uint64_t seed) { return (seed + 1) * 0x9E3779B97F4A7C15ull; }
// replicate b of gene g: gene * reps + b < 2^31 (checked by the callers)
PML_GS_HD uint64_t gs_key(uint64_t base, int gene, int reps, int b) { return base + ((uint64_t)((int64_t)gene * reps + b) << 32); }
// with replacement: draw j of a domain of U indices, rell.hip's rule (no 64-bit division)
PML_GS_HD uint32_t gs_draw(uint64_t key, uint32_t j, uint32_t U) { return (uint32_t)(((gs_mix64(key + j) >> 32) * (uint64_t)U) >> 32); }
// half the bits of the Feistel network over [0, U): max(1, (bitlength(U - 1) + 1) / 2), 1 <= U < 2^31
PML_GS_HD int gs_half_bits(uint32_t U) {
    int bl = 0;
    for (uint32_t v = U - 1; v; v >>= 1) ++bl;
    const int h = (bl + 1) / 2;
    return h < 1 ? 1 : h;
}
// without replacement: a keyed bijection on [0, U).  Four balanced Feistel rounds on 2h bits, cycle-walked back into the domain;
// the walk ends because the network is a permutation of [0, 2^2h) and x starts inside [0, U)
PML_GS_HD uint32_t gs_perm(uint64_t K, uint32_t U, int h, uint32_t x) {
    const uint32_t m = (1u << h) - 1;
    do {
        uint32_t L = x >> h, R = x & m;
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (uint64_t r = 0; r < 4; ++r) {
            const uint32_t F = (uint32_t)gs_mix64(K + (r << 40) + R) & m;
            const uint32_t t = L ^ F;
            L = R; R = t;
        }
        x = (L << h) | R;
    } while (x >= U);
    return x;
}
// the domain index of a gene that is itself part of the table reads T[u] below the gene's start and T[u + len] above it; a
// masked gene (split = U) reads T[u]
PML_GS_HD uint32_t gs_table_index(uint32_t u, uint32_t split, uint32_t len) { return u < split ? u : u + len; }

// ---- host half (genesteps_host.cpp) ----
// what one call of pml_step_thresholds does with every gene: the compact table's columns and every gene's place in it
struct GsPlan {
    int k = 0;                              // (int)ceil(reps * alpha), in [1, reps]
    std::vector<long long> table_cols;      // concatenation column of every table entry: the unmasked genes' columns, in order
    std::vector<uint32_t> split, len, U;    // per gene: its start in the table (U when masked), its columns, its domain
    std::vector<char> run;                  // per gene: 0 = the -1 rule applies, no replicates
};
struct GsOpts { int statistic, replace, multiple, reps; double alpha; unsigned long long seed; const unsigned char *mask; };
// PML_OK, or PML_EINVAL with err filled.  only >= 0: the call is about that gene alone, a domain too small for another gene is no error
int gs_plan(const GsOpts &o, int ngenes, const long long *col_start, int only, GsPlan &plan, std::string &err);
// the concatenation columns replicate `rep` of `gene` draws, in draw order
void gs_draw_columns(const GsOpts &o, const GsPlan &plan, int gene, int rep, long long *cols_out);
// the Java's totals (:65-103) from the two per-column arrays
void gs_totals(int ngenes, const long long *col_start, const int *steps, const int *min_steps, long long *gene_steps, long long *gene_beyond, float *gene_ratio);
// sorts sums ascending; returns sums[reps - k]; n_ge = the sums >= observed
double gs_order_statistic(double *sums, int reps, int k, double observed, long long *n_ge);

}  // namespace pml
