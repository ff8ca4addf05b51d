// gblocks.hip -- the reference's `-gblocks_trim` (MSATrimmer.trim, MSATrimmer.java:41-126: Gblocks -b1 -b3=8 -b5=h) on the device.
// The rule is the published block selection, stated in include/peprml.h; its functions are gblocks.hpp's, shared with the host.
//
// k_gbclass     workgroup = TRIM_COLS columns of one gene, thread = one column, as k_colclass.  No histogram: b1 > n / 2, so a byte
//               that reaches b1 is a strict majority of the column's rows, and then also of its non-gap bytes.  Pass 1 keeps a
//               Boyer-Moore majority candidate over the non-gap bytes and counts '-' and '?'; pass 2 counts the candidate.  If a
//               byte reaches b1 it is the candidate and the count is exact; otherwise the count is below b1 like every other
//               byte's and the class is 0 whatever it is.  A handful of registers for any number of rows, no LDS.  The '-' and
//               '?' cells go to the gene's counter as in k_colclass (integer atomicAdd per wavefront: the order does not matter).
// k_gbselect    one workgroup of GB_CHUNK threads per gene.  Each of the five steps is a predicate on previous / next indices
//               (gblocks.hpp), so a round is a forward pass (inclusive max-scan) and a backward pass (inclusive min-scan) over
//               the gene's columns in chunks of GB_CHUNK, a carry in registers between chunks.  Inside a wavefront the scan is
//               shuffles, across the four wavefronts their totals go through LDS.  Thread t owns columns t, t + GB_CHUNK, ...
//               in both directions, so the column's byte and the forward pass' values are read back by the thread that wrote
//               them; the values live in LDS for a gene of up to GB_LDS_COLS columns, else in the gene's scratch slice.  A last
//               forward pass is the exclusive sum-scan of the kept bits: it writes src_col and nkept / ld_out into the gene's
//               TgGene, which k_colgather reads.  No workgroup waits on another, no atomics.
#include "kernels.h"
#include "trim.hpp"

namespace pml {

__global__ __launch_bounds__(TRIM_COLS) void k_gbclass(const CgGene *__restrict__ genes, const GbGene *__restrict__ gb, const int *__restrict__ tile_gene,
                                                       const int *__restrict__ tile_first, uint8_t *__restrict__ flags, long long *gap_or_missing) {
    const int gi = tile_gene[blockIdx.x];
    const CgGene g = genes[gi];
    const int c = ((int)blockIdx.x - tile_first[gi]) * TRIM_COLS + (int)threadIdx.x;
    const bool active = c < g.ncols;                                   // no early return: every lane takes part in the shuffles
    long long hidden = 0;
    if (active) {
        const GbParams p = gb[gi].p;
        const uint8_t *col = g.bytes + c;                              // c < ncols <= ld: inside every row
        unsigned cand = 256;                                           // no byte yet
        int weight = 0, gaps = 0, missing = 0;
#pragma unroll 4
        for (int r = 0; r < g.ntax; ++r) {
            const unsigned b = col[(size_t)r * g.ld];
            const bool gap = b == '-';
            gaps += gap; missing += b == '?';
            if (!gap) {
                if (weight == 0) cand = b;
                weight += (weight == 0 || b == cand) ? 1 : -1;
            }
        }
        int top = 0;
#pragma unroll 4
        for (int r = 0; r < g.ntax; ++r) top += col[(size_t)r * g.ld] == cand;
        flags[g.col_base + c] = (uint8_t)gb_class(gaps, top, g.ntax, p);
        hidden = gaps + missing;
    }
    for (int off = 32; off > 0; off >>= 1) hidden += __shfl_xor(hidden, off);
    if ((threadIdx.x & 63) == 0 && hidden) atomicAdd((unsigned long long *)&gap_or_missing[gi], (unsigned long long)hidden);
}

constexpr int GB_WAVES = GB_CHUNK / 64;

// inclusive scan of two values over the workgroup's GB_CHUNK threads, the carry of the chunks before folded in and updated.
// FWD: prefix maximum in thread order; else suffix minimum.  tot: 2 * GB_WAVES ints of LDS; two barriers.
template <bool FWD> __device__ __forceinline__ void gb_scan2(int &a, int &b, int &carry_a, int &carry_b, int *tot) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int ta = FWD ? __shfl_up(a, off) : __shfl_down(a, off), tb = FWD ? __shfl_up(b, off) : __shfl_down(b, off);
        if (FWD ? lane >= off : lane + off < 64) { a = FWD ? max(a, ta) : min(a, ta); b = FWD ? max(b, tb) : min(b, tb); }
    }
    if (lane == (FWD ? 63 : 0)) { tot[wave] = a; tot[GB_WAVES + wave] = b; }
    __syncthreads();
    int ea = carry_a, eb = carry_b;                                    // what the chunks and wavefronts before this one give
#pragma unroll
    for (int w = 0; w < GB_WAVES; ++w) {
        const int ta = tot[w], tb = tot[GB_WAVES + w];
        if (FWD ? w < wave : w > wave) { ea = FWD ? max(ea, ta) : min(ea, ta); eb = FWD ? max(eb, tb) : min(eb, tb); }
        carry_a = FWD ? max(carry_a, ta) : min(carry_a, ta); carry_b = FWD ? max(carry_b, tb) : min(carry_b, tb);
    }
    a = FWD ? max(a, ea) : min(a, ea); b = FWD ? max(b, eb) : min(b, eb);
    __syncthreads();                                                   // tot is written again by the next scan
}

__global__ __launch_bounds__(GB_CHUNK) void k_gbselect(const GbGene *__restrict__ genes, uint8_t *flags, TgGene *tg) {
    __shared__ int lds_prev[2 * GB_LDS_COLS];
    __shared__ int tot[2 * GB_WAVES];
    const GbGene g = genes[blockIdx.x];
    const int L = g.ncols, t = (int)threadIdx.x;
    uint8_t *f = flags + g.col_base;
    int *prev_a = L <= GB_LDS_COLS ? lds_prev : g.scratch, *prev_b = prev_a + L;       // scratch holds 2 * ncols ints
    const int nchunks = (L + GB_CHUNK - 1) / GB_CHUNK;
    for (int r = 1; r <= GB_ROUNDS; ++r) {
        int carry_a = -1, carry_b = -1;
        for (int k = 0; k < nchunks; ++k) {                            // every thread runs every chunk: the scans hold barriers
            const int c = k * GB_CHUNK + t;
            bool A = false, B = false;
            if (c < L) gb_round_in(r, f[c], A, B);
            int a = A ? c : -1, b = B ? c : -1;
            gb_scan2<true>(a, b, carry_a, carry_b, tot);
            if (c < L) { prev_a[c] = a; prev_b[c] = b; }
        }
        carry_a = L; carry_b = L;
        for (int k = nchunks - 1; k >= 0; --k) {
            const int c = k * GB_CHUNK + t;
            bool A = false, B = false;
            unsigned fc = 0;
            if (c < L) { fc = f[c]; gb_round_in(r, fc, A, B); }
            int a = A ? c : L, b = B ? c : L;
            gb_scan2<false>(a, b, carry_a, carry_b, tot);
            if (c < L) f[c] = (uint8_t)gb_round_out(r, fc, prev_a[c], prev_b[c], a, b, g.p);       // this thread's own column
        }
    }
    // the kept columns, ascending: an exclusive sum-scan of the kept bits
    int base = 0;
    for (int k = 0; k < nchunks; ++k) {
        const int c = k * GB_CHUNK + t, lane = t & 63, wave = t >> 6;
        const bool kept = c < L && (f[c] & GB_KEPT);
        const unsigned long long m = __ballot(kept);
        if (lane == 0) tot[wave] = __popcll(m);
        __syncthreads();
        int at = base + __popcll(m & ((1ull << lane) - 1));
#pragma unroll
        for (int w = 0; w < GB_WAVES; ++w) { if (w < wave) at += tot[w]; base += tot[w]; }
        if (kept) g.src_col[at] = c;                                   // at < nkept <= ncols <= ld, src_col's length
        __syncthreads();
    }
    const int ld_out = (base + 15) & ~15;                              // <= ld: ld is ncols rounded up to 16
    if (base + t < ld_out) g.src_col[base + t] = -1;                   // at most 15 entries
    if (t == 0) { tg[blockIdx.x].nkept = base; tg[blockIdx.x].ld_out = ld_out; }
}

void launch_gbclass(const CgGene *genes, const GbGene *gb, const int *tile_gene, const int *tile_first, int ntiles, uint8_t *flags,
                    long long *gap_or_missing, hipStream_t s) {
    if (ntiles <= 0) return;
    hipLaunchKernelGGL(k_gbclass, dim3((unsigned)ntiles), dim3(TRIM_COLS), 0, s, genes, gb, tile_gene, tile_first, flags, gap_or_missing);
}

void launch_gbselect(const GbGene *gb, int ngenes, uint8_t *flags, TgGene *tg, hipStream_t s) {
    if (ngenes <= 0) return;
    hipLaunchKernelGGL(k_gbselect, dim3((unsigned)ngenes), dim3(GB_CHUNK), 0, s, gb, flags, tg);
}

}  // namespace pml
