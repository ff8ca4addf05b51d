// genesteps.hip -- the gene homoplasy test of ConcatenatedSequenceAlignment.java:65-425 on the device: per-column Fitch steps of
// the concatenation on a tree, the least steps a column can take, and the resampler behind the per-gene thresholds.  The rules
// are in include/peprml.h, the draw functions in genesteps.hpp (shared with the host), the host half in genesteps.cpp.
//
// k_fitch_sitesteps  thread = one pattern of the replicate of all genes of a sub-batch (tip rows by k_fitch_tips).  It walks the
//               tree's post-order SET list as k_fitch does, re-reading only what it wrote itself, counts its own unions in a
//               register and stores one count.  No wave reduction, no atomics, no barrier.
// k_steps_expand     thread = one column: steps[column] = the count of the column's pattern, through the gene's site2pat.
// k_colminsteps      thread = one column over the gene's own rows of raw bytes, every byte read once; the bytes seen (and seen
//               twice: trim.hpp's trim_note, the state k_colclass keeps) are two 256-bit masks in registers.  Stores
//               classes - 1 - [classes == 2 and shown == n], n = the union's taxa; -1 for a column of only '-' and '?'.
// k_steps_table      the compact table of the chosen statistic over the unmasked genes' columns: steps, steps - min_steps, or
//               (float)steps / (float)(min_steps + 1), one correctly rounded division.
// k_steps_resample   thread = one replicate of one gene; a workgroup, so a wavefront, holds replicates of ONE gene and its lanes run
//               the same trip count.  Each draw is a hash (with replacement) or four (a Feistel permutation, without) and one
//               gather from the table, added in ascending draw order in a register: int sums are exact, float sums are the
//               Java's sequential chain.  One store per replicate; no atomics, no barrier, nothing waits.  Every index is
//               bounded by the descriptor: u < U, and U + len <= the table's entries for a gene that is part of the table.
#include "fitch_dev.hpp"
#include "genesteps.hpp"
#include "kernels.h"
#include "trim.hpp"

namespace pml {

__global__ __launch_bounds__(256) void k_fitch_sitesteps(const GsOp *__restrict__ ops, int nops, unsigned *pool, int mpad, int npat, int *__restrict__ pat_steps) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= npat) return;                                         // npat <= mpad; no barrier follows
    const size_t m = (size_t)mpad;
    int count = 0;
    for (int i = 0; i < nops; ++i) {
        const GsOp op = ops[i];                                    // uniform -> scalar loads
        const unsigned l = pool[op.l * m + p], r = pool[op.r * m + p];
        count += (l & r) == 0;
        if (op.out >= 0) pool[op.out * m + p] = fitch(l, r);
    }
    pat_steps[p] = count;
}

__global__ __launch_bounds__(GS_COLS) void k_steps_expand(const GsGene *__restrict__ genes, const int *__restrict__ tile_gene, const int *__restrict__ tile_first,
                                                          const int *__restrict__ pat_steps, int *__restrict__ steps) {
    const int gi = tile_gene[blockIdx.x];
    const GsGene g = genes[gi];
    const int c = ((int)blockIdx.x - tile_first[gi]) * GS_COLS + (int)threadIdx.x;
    if (c >= g.ncols) return;
    steps[g.col_base + c] = pat_steps[g.pat_off + g.site2pat[c]];  // site2pat[c] < the gene's patterns
}

__global__ __launch_bounds__(GS_COLS) void k_colminsteps(const GsGene *__restrict__ genes, const int *__restrict__ tile_gene, const int *__restrict__ tile_first,
                                                         int n_union, int *__restrict__ min_steps) {
    const int gi = tile_gene[blockIdx.x];
    const GsGene g = genes[gi];
    const int c = ((int)blockIdx.x - tile_first[gi]) * GS_COLS + (int)threadIdx.x;
    if (c >= g.ncols) return;
    uint32_t seen1[8] = {0, 0, 0, 0, 0, 0, 0, 0}, seen2[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int shown = 0;
    const uint8_t *p = g.bytes + c;                                // c < ncols <= ld: inside every row
#pragma unroll 4
    for (int r = 0; r < g.ntax; ++r) trim_note(seen1, seen2, shown, p[(size_t)r * g.ld]);
    constexpr uint32_t GAP = 1u << ('-' & 31), MISSING = 1u << ('?' & 31);      // both in word 1
    const int classes = trim_popcount(seen1) - ((seen1[1] & GAP) != 0) - ((seen1[1] & MISSING) != 0);
    // the rows the gene lacks are '?': shown == n needs every taxon of the union
    min_steps[g.col_base + c] = classes - 1 - (classes == 2 && shown == n_union);
}

template <typename T>
__global__ __launch_bounds__(256) void k_steps_table(const int *__restrict__ steps, const int *__restrict__ mins, long long n, int statistic, T *__restrict__ table) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int s = steps[i], m = mins[i];
    if (statistic == GS_RATIO) table[i] = (T)((float)s / (float)(m + 1));
    else table[i] = (T)(statistic == GS_BEYOND ? s - m : s);
}

template <typename T, bool REPLACE>
__global__ __launch_bounds__(256) void k_steps_resample(const GsEntry *__restrict__ entries, const T *__restrict__ table, T *__restrict__ sums, int reps,
                                                        unsigned long long base, int blocks_per_gene) {
    const int ei = (int)(blockIdx.x / (unsigned)blocks_per_gene);
    const GsEntry e = entries[ei];                                 // uniform over the workgroup
    const int b = (int)(blockIdx.x % (unsigned)blocks_per_gene) * 256 + (int)threadIdx.x;
    if (b >= reps) return;
    const uint64_t key = gs_key(base, e.gene, reps, b);
    T acc = 0;
    if (REPLACE) {
        for (uint32_t j = 0; j < e.len; ++j) acc += table[gs_table_index(gs_draw(key, j, e.U), e.split, e.len)];
    } else {
        const uint64_t K = gs_mix64(key);
        const int h = gs_half_bits(e.U);
        for (uint32_t j = 0; j < e.len; ++j) acc += table[gs_table_index(gs_perm(K, e.U, h, j), e.split, e.len)];      // j < len <= U
    }
    sums[(size_t)ei * reps + b] = acc;
}

void launch_fitch_sitesteps(const GsOp *ops, int nops, unsigned *pool, int mpad, int npat, int *pat_steps, hipStream_t s) {
    if (npat <= 0) return;
    hipLaunchKernelGGL(k_fitch_sitesteps, dim3((unsigned)((npat + 255) / 256)), dim3(256), 0, s, ops, nops, pool, mpad, npat, pat_steps);
}
void launch_steps_expand(const GsGene *genes, const int *tile_gene, const int *tile_first, int ntiles, const int *pat_steps, int *steps, hipStream_t s) {
    if (ntiles <= 0) return;
    hipLaunchKernelGGL(k_steps_expand, dim3((unsigned)ntiles), dim3(GS_COLS), 0, s, genes, tile_gene, tile_first, pat_steps, steps);
}
void launch_colminsteps(const GsGene *genes, const int *tile_gene, const int *tile_first, int ntiles, int n_union, int *min_steps, hipStream_t s) {
    if (ntiles <= 0) return;
    hipLaunchKernelGGL(k_colminsteps, dim3((unsigned)ntiles), dim3(GS_COLS), 0, s, genes, tile_gene, tile_first, n_union, min_steps);
}
void launch_steps_table(const int *steps, const int *mins, long long n, int statistic, void *table, hipStream_t s) {
    if (n <= 0) return;
    const dim3 grid((unsigned)((n + 255) / 256));
    if (statistic == GS_RATIO) hipLaunchKernelGGL(k_steps_table<float>, grid, dim3(256), 0, s, steps, mins, n, statistic, (float *)table);
    else hipLaunchKernelGGL(k_steps_table<int>, grid, dim3(256), 0, s, steps, mins, n, statistic, (int *)table);
}
void launch_steps_resample(const GsEntry *entries, int nentries, const void *table, void *sums, int reps, unsigned long long base, bool as_float, bool replace, hipStream_t s) {
    if (nentries <= 0 || reps <= 0) return;
    const int bpg = (reps + 255) / 256;
    const dim3 grid((unsigned)((long long)nentries * bpg));        // < 2^31 / 256 + nentries: ngenes * reps < 2^31
    if (as_float) {
        if (replace) hipLaunchKernelGGL((k_steps_resample<float, true>), grid, dim3(256), 0, s, entries, (const float *)table, (float *)sums, reps, base, bpg);
        else hipLaunchKernelGGL((k_steps_resample<float, false>), grid, dim3(256), 0, s, entries, (const float *)table, (float *)sums, reps, base, bpg);
    } else {
        if (replace) hipLaunchKernelGGL((k_steps_resample<int, true>), grid, dim3(256), 0, s, entries, (const int *)table, (int *)sums, reps, base, bpg);
        else hipLaunchKernelGGL((k_steps_resample<int, false>), grid, dim3(256), 0, s, entries, (const int *)table, (int *)sums, reps, base, bpg);
    }
}

}  // namespace pml
