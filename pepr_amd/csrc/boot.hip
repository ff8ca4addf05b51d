// boot.hip -- the column bootstrap's replicates, built on the device from the genes resident in HBM (boot.hpp: the draw rule).
//
//   k_boot_count   count[r][p] = the draws of replicate r that land on a column of pattern p
//   k_boot_index   idx[r][0..npat_r) = the patterns with count > 0, ascending (stable compaction)
//   k_boot_gather  the replicate's code matrix with f64 weights (an ML batch) or its Fitch state sets with int weights (a pool)
//   k_boot_pairs   the weighted comparable / differing counts of every taxon pair of the replicate's code matrix
//
// All integer work: every result is a sum of integers or a copy, so the bytes do not depend on the schedule.  No kernel waits on
// another workgroup; every index is bounded by a descriptor (BootSpace, BootRep) the host filled.
#include "boot_dev.hpp"
#include "fitch_dev.hpp"

namespace pml {

// blockIdx.y = replicate, blockIdx.x = a chunk of BOOT_CHUNK draws.  The hash is ALU work, col2pat is L ints read at random
// (L2-resident: 4 B per column), the histogram is LDS atomics; latency-bound, small.  LDS form: the workgroup's histogram of P <=
// BOOT_LDS_BINS bins, flushed with plain stores when it is the replicate's only workgroup, else with one global add per non-empty
// bin.  Global form (k_boot_count_global: P larger, or PML_BOOT_GLOBAL_HIST=1; a kernel of its own, so it holds no LDS): one
// global add per draw.  Both forms add into count[r], which the host zeroed.  Integer adds commute: both forms give the same bytes.
__global__ __launch_bounds__(256) void k_boot_count_global(const BootSpace sp, const BootRep *__restrict__ reps) {
    const BootRep rep = reps[blockIdx.y];
    const unsigned j0 = blockIdx.x * (unsigned)BOOT_CHUNK;                  // < L: the grid has ceil(L / BOOT_CHUNK) chunks
    const unsigned j1 = sp.L - j0 < (unsigned)BOOT_CHUNK ? sp.L : j0 + BOOT_CHUNK;
    for (unsigned j = j0 + threadIdx.x; j < j1; j += 256) atomicAdd(&rep.count[sp.col2pat[boot_draw(rep.key, j, sp.L)]], 1u);
}
__global__ __launch_bounds__(256) void k_boot_count(const BootSpace sp, const BootRep *__restrict__ reps) {
    __shared__ unsigned hist[BOOT_LDS_BINS];
    const BootRep rep = reps[blockIdx.y];
    const unsigned j0 = blockIdx.x * (unsigned)BOOT_CHUNK;
    const unsigned j1 = sp.L - j0 < (unsigned)BOOT_CHUNK ? sp.L : j0 + BOOT_CHUNK;
    for (int p = threadIdx.x; p < sp.P; p += 256) hist[p] = 0;
    __syncthreads();
    for (unsigned j = j0 + threadIdx.x; j < j1; j += 256) atomicAdd(&hist[sp.col2pat[boot_draw(rep.key, j, sp.L)]], 1u);
    __syncthreads();
    if (gridDim.x == 1) { for (int p = threadIdx.x; p < sp.P; p += 256) rep.count[p] = hist[p]; return; }
    for (int p = threadIdx.x; p < sp.P; p += 256) if (hist[p]) atomicAdd(&rep.count[p], hist[p]);
}

// One workgroup per replicate walks count[r] in tiles of BOOT_TILE patterns, a pattern per thread: ballot + popcount inside a
// wavefront, the four wave totals through LDS, and the running offset carried from tile to tile in a register every thread holds.
__global__ __launch_bounds__(BOOT_TILE) void k_boot_index(const BootSpace sp, const BootRep *__restrict__ reps) {
    __shared__ int wave_total[BOOT_TILE / 64];
    const BootRep rep = reps[blockIdx.x];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int base = 0;
    for (int t0 = 0; t0 < sp.P; t0 += BOOT_TILE) {
        const int p = t0 + threadIdx.x;
        const bool live = p < sp.P && rep.count[p] != 0;
        const unsigned long long b = __ballot(live);
        if (lane == 0) wave_total[wave] = __popcll(b);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < BOOT_TILE / 64; ++w) { const int c = wave_total[w]; before += w < wave ? c : 0; total += c; }
        if (live) rep.idx[base + before + __popcll(b & ((1ull << lane) - 1ull))] = p;      // < P: one slot per live pattern so far
        base += total;
        __syncthreads();                                         // wave_total is rewritten by the next tile
    }
    if (threadIdx.x == 0) *rep.npat_dev = base;
}

// the gene of pattern p: the last segment that starts at or before it (segments ascend in pat_off, segs[0].pat_off = 0)
__device__ __forceinline__ int boot_seg_of(const BootSpace &sp, int p) {
    int lo = 0, hi = sp.nseg - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (sp.segs[mid].pat_off <= p) lo = mid; else hi = mid - 1; }
    return lo;
}

// blockIdx.y = replicate, a thread per compact position q < mpad; rows are walked in a loop, so a wavefront stores 64 (codes) or
// 256 (state sets) contiguous bytes per row, as k_gather and k_fitch_tips do.  q >= npat is padding: the gap code or every state,
// weight 0.  Byte reads through idx (random within the genes' matrices), HBM / L2-bound.
template <int FORM>
__global__ __launch_bounds__(256) void k_boot_gather(const BootSpace sp, const BootRep *__restrict__ reps) {
    const BootRep rep = reps[blockIdx.y];
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= rep.mpad) return;
    const bool live = q < rep.npat;                              // npat <= P: idx[q] was written
    int p = 0, local = 0, seg = 0; unsigned w = 0;
    if (live) { p = rep.idx[q]; seg = boot_seg_of(sp, p); local = p - sp.segs[seg].pat_off; w = rep.count[p]; }
    const BootSeg sg = sp.segs[seg];
    const int *rowmap = sp.rowmaps + (size_t)seg * sp.ntax;
    if (FORM == BOOT_FORM_CODES) ((double *)rep.dst_w)[q] = (double)w; else ((int *)rep.dst_w)[q] = (int)w;
    for (int t = 0; t < sp.ntax; ++t) {
        const int row = live ? rowmap[t] : -1;
        const int code = row >= 0 ? sg.src[(size_t)row * sg.src_mpad + local] : NCODES - 1;
        if (FORM == BOOT_FORM_CODES) ((uint8_t *)rep.dst)[(size_t)t * rep.mpad + q] = (uint8_t)code;
        else ((unsigned *)rep.dst)[(size_t)t * rep.mpad + q] = code_mask(code);
    }
}

// blockIdx.y = replicate, blockIdx.x = taxon i; wave w of the workgroup takes the partners j = i + 1 + w, i + 5 + w, ...: its
// lanes stride the replicate's patterns, the two sums are folded across the wavefront by shuffles and lane 0 stores both halves of
// the symmetric tables.  pair_counts (host.cpp) with the replicate's weights, in int64.  The matrix of a replicate is read ntax
// times from L2; integer compares, tiny next to a search.
__global__ __launch_bounds__(256) void k_boot_pairs(const BootSpace sp, const BootRep *__restrict__ reps) {
    const BootRep rep = reps[blockIdx.y];
    const int i = blockIdx.x, lane = threadIdx.x & 63, n = sp.ntax;
    const uint8_t *codes = (const uint8_t *)rep.dst;
    const double *wgt = (const double *)rep.dst_w;
    const uint8_t *ci = codes + (size_t)i * rep.mpad;
    for (int j = i + 1 + (int)(threadIdx.x >> 6); j < n; j += 4) {
        const uint8_t *cj = codes + (size_t)j * rep.mpad;
        long long c = 0, d = 0;
        for (int q = lane; q < rep.npat; q += 64) {
            const int a = ci[q], b = cj[q];
            const long long w = (a < NS && b < NS) ? (long long)wgt[q] : 0;
            c += w; d += a != b ? w : 0;
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) { c += __shfl_xor(c, m, 64); d += __shfl_xor(d, m, 64); }
        if (lane == 0) {
            rep.cmp[(size_t)i * n + j] = c; rep.cmp[(size_t)j * n + i] = c;
            rep.diff[(size_t)i * n + j] = d; rep.diff[(size_t)j * n + i] = d;
        }
    }
}

void launch_boot_count(const BootSpace &sp, const BootRep *reps, int nreps, bool global_form, hipStream_t s) {
    if (nreps <= 0) return;
    const unsigned chunks = (sp.L + BOOT_CHUNK - 1) / BOOT_CHUNK;
    if (global_form || sp.P > BOOT_LDS_BINS) hipLaunchKernelGGL(k_boot_count_global, dim3(chunks, (unsigned)nreps), dim3(256), 0, s, sp, reps);
    else hipLaunchKernelGGL(k_boot_count, dim3(chunks, (unsigned)nreps), dim3(256), 0, s, sp, reps);
}
void launch_boot_index(const BootSpace &sp, const BootRep *reps, int nreps, hipStream_t s) {
    if (nreps <= 0) return;
    hipLaunchKernelGGL(k_boot_index, dim3((unsigned)nreps), dim3(BOOT_TILE), 0, s, sp, reps);
}
void launch_boot_gather(const BootSpace &sp, const BootRep *reps, int nreps, int max_mpad, int form, hipStream_t s) {
    if (nreps <= 0 || max_mpad <= 0) return;
    const dim3 grid((unsigned)((max_mpad + 255) / 256), (unsigned)nreps);
    if (form == BOOT_FORM_CODES) hipLaunchKernelGGL(k_boot_gather<BOOT_FORM_CODES>, grid, dim3(256), 0, s, sp, reps);
    else hipLaunchKernelGGL(k_boot_gather<BOOT_FORM_MASKS>, grid, dim3(256), 0, s, sp, reps);
}
void launch_boot_pairs(const BootSpace &sp, const BootRep *reps, int nreps, hipStream_t s) {
    if (nreps <= 0) return;
    hipLaunchKernelGGL(k_boot_pairs, dim3((unsigned)sp.ntax, (unsigned)nreps), dim3(256), 0, s, sp, reps);
}

}  // namespace pml
