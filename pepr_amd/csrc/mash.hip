// mash.hip -- the MinHash path's kernels (include/peprml.h "NeighborMasher"): k_mash_hash (window values, valid counts and the cut
// histogram), k_mash_cut (the cut of every genome from its histogram), k_mash_compact (the values under the cut), k_mash_unique
// (the sorted survivors to a sketch) and k_mash_pairs (common / denom of every pair of a block of resident sketches).  The
// survivors are sorted between k_mash_compact and k_mash_unique by rocPRIM's segmented radix sort (launch_mash_sort).
#include <hip/hip_runtime.h>
#include <cstring>
#include <rocprim/device/device_segmented_radix_sort.hpp>

#include "kernels.h"

namespace pml {

namespace {

// One workgroup = one span: up to MASH_SPAN_TILES tiles of MASH_TILE window starts of ONE genome.  A tile and its k - 1 halo are
// staged in LDS; thread t takes the starts t, t + 256, t + 512, t + 768 of the tile, so a wave's stores are contiguous.
__global__ __launch_bounds__(MASH_THREADS) void k_mash_hash(const uint8_t *bytes, unsigned nbytes, const MashSpan *spans, int k, uint64_t *values,
                                                            unsigned long long *nvalid, unsigned *hist) {
    __shared__ uint8_t l_tile[MASH_TILE + 32];
    __shared__ unsigned l_hist[MASH_BINS];
    __shared__ unsigned l_valid;
    const MashSpan sp = spans[blockIdx.x];
    const int t = threadIdx.x;
    for (int b = t; b < MASH_BINS; b += MASH_THREADS) l_hist[b] = 0;
    if (t == 0) l_valid = 0;
    const int shift = mash_value_bits(k) - MASH_BIN_BITS;
    unsigned mine = 0;
    for (unsigned t0 = sp.begin; t0 < sp.end; t0 += MASH_TILE) {
        __syncthreads();                                           // the tile before is read, and the histogram is zero
        for (int i = t; i < MASH_TILE + k - 1; i += MASH_THREADS) {
            const unsigned at = t0 + (unsigned)i;
            l_tile[i] = at < sp.end + (unsigned)(k - 1) && at < nbytes ? bytes[at] : MASH_SEP;     // a genome ends in a separator
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < MASH_TILE / MASH_THREADS; ++q) {
            const int w = t + q * MASH_THREADS;
            const unsigned at = t0 + (unsigned)w;
            if (at >= sp.end) continue;
            uint64_t fw = 0, rc = 0;
            unsigned bad = 0;
            for (int j = 0; j < k; ++j) {
                const unsigned c = mash_code(l_tile[w + j]);
                bad |= c >> 2;
                fw = (fw << 2) | (c & 3u);
                rc = (rc >> 2) | ((uint64_t)(3u - (c & 3u)) << (2 * (k - 1)));
            }
            uint64_t v = MASH_INVALID;
            if (!bad) {
                v = mash_value(fw, rc, k);
                if (v != MASH_INVALID) { ++mine; atomicAdd(&l_hist[(unsigned)(v >> shift)], 1u); }
            }
            values[at] = v;
        }
    }
    atomicAdd(&l_valid, mine);
    __syncthreads();
    unsigned *gh = hist + (size_t)sp.genome * MASH_BINS;
    for (int b = t; b < MASH_BINS; b += MASH_THREADS) { const unsigned c = l_hist[b]; if (c) atomicAdd(&gh[b], c); }
    if (t == 0 && l_valid) atomicAdd(&nvalid[sp.genome], (unsigned long long)l_valid);
}

// One workgroup per genome: the smallest number of leading bins that holds at least s + s / 16 + 64 valid windows (all bins when
// there are fewer), not below min_bins (what a repeat asks for).  Also clears the genome's survivor count.
__global__ __launch_bounds__(256) void k_mash_cut(const unsigned *hist, const unsigned long long *nvalid, const int *min_bins, int s, int *cut_bins,
                                                  unsigned *count) {
    __shared__ unsigned long long l_sum[256];
    __shared__ int l_cut;
    const int g = blockIdx.x, t = threadIdx.x;
    const unsigned *h = hist + (size_t)g * MASH_BINS;
    constexpr int PER = MASH_BINS / 256;
    unsigned long long own = 0;
    for (int b = 0; b < PER; ++b) own += h[t * PER + b];
    l_sum[t] = own;
    if (t == 0) l_cut = MASH_BINS;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {                            // inclusive scan
        const unsigned long long add = t >= d ? l_sum[t - d] : 0;
        __syncthreads();
        l_sum[t] += add;
        __syncthreads();
    }
    const unsigned long long target = (unsigned long long)s + (unsigned long long)(s / 16) + 64;
    unsigned long long before = l_sum[t] - own;
    if (before < target && target <= before + own) {               // at most one thread
        int b = 0;
        for (; b < PER; ++b) { before += h[t * PER + b]; if (before >= target) break; }
        l_cut = t * PER + b + 1;
    }
    __syncthreads();
    if (t == 0) {
        int c = l_cut;
        if (nvalid[g] < target) c = MASH_BINS;
        if (c < min_bins[g]) c = min_bins[g];
        if (c > MASH_BINS) c = MASH_BINS;
        cut_bins[g] = c;
        count[g] = 0;
    }
}

// The spans of k_mash_hash again: every value under its genome's cut goes to comp[first[genome] + ...], in no particular order
// (a sort follows).  One atomic per tile reserves the tile's room.
__global__ __launch_bounds__(MASH_THREADS) void k_mash_compact(const uint64_t *values, const MashSpan *spans, const unsigned *first, const int *cut_bins, int k,
                                                               uint64_t *comp, unsigned *count) {
    constexpr int Q = MASH_TILE / MASH_THREADS, WAVES = MASH_THREADS / 64;
    __shared__ unsigned l_off[Q * WAVES + 1];
    const MashSpan sp = spans[blockIdx.x];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int cb = cut_bins[sp.genome];
    const int shift = mash_value_bits(k) - MASH_BIN_BITS;
    const bool all = cb >= MASH_BINS;
    const uint64_t cut = all ? 0 : (uint64_t)cb << shift;
    const unsigned base_g = first[sp.genome];
    for (unsigned t0 = sp.begin; t0 < sp.end; t0 += MASH_TILE) {
        uint64_t v[Q];
        unsigned rank[Q];
        bool keep[Q];
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const unsigned at = t0 + (unsigned)(t + q * MASH_THREADS);
            v[q] = at < sp.end ? values[at] : MASH_INVALID;
            keep[q] = v[q] != MASH_INVALID && (all || v[q] < cut);
            const unsigned long long m = __ballot(keep[q]);
            rank[q] = (unsigned)__popcll(m & ((1ull << lane) - 1ull));
            if (lane == 0) l_off[q * WAVES + wave] = (unsigned)__popcll(m);
        }
        __syncthreads();
        if (t == 0) {
            unsigned run = 0;
            for (int i = 0; i < Q * WAVES; ++i) { const unsigned c = l_off[i]; l_off[i] = run; run += c; }
            const unsigned got = run ? atomicAdd(&count[sp.genome], run) : 0u;
            l_off[Q * WAVES] = got;
        }
        __syncthreads();
        const unsigned tile_base = base_g + l_off[Q * WAVES];
#pragma unroll
        for (int q = 0; q < Q; ++q)
            if (keep[q]) comp[tile_base + l_off[q * WAVES + wave] + rank[q]] = v[q];
        __syncthreads();                                           // l_off is rewritten by the next tile
    }
}

__global__ void k_mash_segments(const unsigned *first, const unsigned *count, int n, unsigned *seg_end) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g < n) seg_end[g] = first[g] + count[g];
}

// One workgroup per genome: the distinct values of its sorted survivors, ascending, the first s of them, to sketch[g][..]; len[g] =
// how many.  Stops as soon as s are written.
__global__ __launch_bounds__(256) void k_mash_unique(const uint64_t *sorted, const unsigned *first, const unsigned *count, int s, uint64_t *sketch, int *len) {
    __shared__ unsigned l_scan[256];
    __shared__ unsigned l_total;
    const int g = blockIdx.x, t = threadIdx.x;
    const uint64_t *v = sorted + first[g];
    const unsigned n = count[g];
    uint64_t *out = sketch + (size_t)g * s;
    unsigned written = 0;
    for (unsigned c0 = 0; c0 < n && written < (unsigned)s; c0 += 256) {
        const unsigned i = c0 + (unsigned)t;
        const uint64_t x = i < n ? v[i] : 0;
        const unsigned flag = i < n && (i == 0 || v[i - 1] != x) ? 1u : 0u;
        l_scan[t] = flag;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {
            const unsigned add = t >= d ? l_scan[t - d] : 0;
            __syncthreads();
            l_scan[t] += add;
            __syncthreads();
        }
        const unsigned at = written + l_scan[t] - flag;
        if (flag && at < (unsigned)s) out[at] = x;
        if (t == 255) l_total = l_scan[255];
        __syncthreads();
        written += l_total;
        __syncthreads();
    }
    if (t == 0) len[g] = written < (unsigned)s ? (int)written : s;
}

__device__ __forceinline__ unsigned mash_lower_bound(const uint64_t *b, unsigned lo, unsigned hi, uint64_t x) {
    while (lo < hi) {
        const unsigned mid = lo + ((hi - lo) >> 1);
        if (b[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// Workgroup (col, row) = the pair (rows[row], cols[col]) of resident sketches a, b (ascending, distinct).  The union rank of a[i]
// is i + |{b < a[i]}| - |{shared values < a[i]}|: a binary search per value and a prefix count of the shared ones, MASH_CHUNK values
// of a at a time.  common = the shared values of rank < s; denom = s once a rank >= s is met, else min(s, |a| + |b| - shared).
__global__ __launch_bounds__(MASH_CHUNK) void k_mash_pairs(const uint64_t *sketch, const int *len, const int *rows, const int *cols, int ncols, int s, int2 *out) {
    __shared__ unsigned l_scan[MASH_CHUNK];
    __shared__ unsigned l_common, l_past, l_lb;
    const int t = threadIdx.x;
    const int ga = rows[blockIdx.y], gb = cols[blockIdx.x];
    const uint64_t *a = sketch + (size_t)ga * s, *b = sketch + (size_t)gb * s;
    const unsigned na = (unsigned)len[ga], nb = (unsigned)len[gb];
    if (t == 0) { l_common = 0; l_past = 0; l_lb = 0; }
    __syncthreads();
    unsigned shared_before = 0, lo = 0;
    bool past = false;
    for (unsigned c0 = 0; c0 < na && !past; c0 += MASH_CHUNK) {
        const unsigned i = c0 + (unsigned)t;
        unsigned lb = 0, eq = 0;
        if (i < na) {
            const uint64_t x = a[i];
            lb = mash_lower_bound(b, lo, nb, x);
            eq = lb < nb && b[lb] == x ? 1u : 0u;
        }
        l_scan[t] = eq;
        __syncthreads();
        for (int d = 1; d < MASH_CHUNK; d <<= 1) {
            const unsigned add = t >= d ? l_scan[t - d] : 0;
            __syncthreads();
            l_scan[t] += add;
            __syncthreads();
        }
        if (i < na) {
            const unsigned long long rank = (unsigned long long)i + lb - (shared_before + l_scan[t] - eq);
            if (rank >= (unsigned long long)s) l_past = 1;         // benign race: every writer stores 1
            else if (eq) atomicAdd(&l_common, 1u);
            if (i == na - 1 || t == MASH_CHUNK - 1) l_lb = lb;     // the next chunk's values are larger: its searches start here
        }
        __syncthreads();
        shared_before += l_scan[MASH_CHUNK - 1];
        past = l_past != 0;
        lo = l_lb;
        __syncthreads();
    }
    if (t == 0) {
        const unsigned long long uni = (unsigned long long)na + nb - shared_before;
        const int denom = past ? s : (int)(uni < (unsigned long long)s ? uni : (unsigned long long)s);
        out[(size_t)blockIdx.y * ncols + blockIdx.x] = make_int2((int)l_common, denom);
    }
}

}  // namespace

void launch_mash_hash(const uint8_t *bytes, unsigned nbytes, const MashSpan *spans, int nspans, int k, uint64_t *values, unsigned long long *nvalid, unsigned *hist,
                      hipStream_t s) {
    if (nspans <= 0) return;
    hipLaunchKernelGGL(k_mash_hash, dim3((unsigned)nspans), dim3(MASH_THREADS), 0, s, bytes, nbytes, spans, k, values, nvalid, hist);
}

void launch_mash_cut(const unsigned *hist, const unsigned long long *nvalid, const int *min_bins, int ngenomes, int s, int *cut_bins, unsigned *count, hipStream_t st) {
    if (ngenomes <= 0) return;
    hipLaunchKernelGGL(k_mash_cut, dim3((unsigned)ngenomes), dim3(256), 0, st, hist, nvalid, min_bins, s, cut_bins, count);
}

void launch_mash_compact(const uint64_t *values, const MashSpan *spans, int nspans, const unsigned *first, const int *cut_bins, int k, uint64_t *comp, unsigned *count,
                         hipStream_t s) {
    if (nspans <= 0) return;
    hipLaunchKernelGGL(k_mash_compact, dim3((unsigned)nspans), dim3(MASH_THREADS), 0, s, values, spans, first, cut_bins, k, comp, count);
}

hipError_t launch_mash_sort(void *tmp, size_t &tmp_bytes, const uint64_t *comp, uint64_t *sorted, unsigned total, int ngenomes, const unsigned *first,
                            const unsigned *count, unsigned *seg_end, int k, hipStream_t s) {
    if (tmp && ngenomes > 0) hipLaunchKernelGGL(k_mash_segments, dim3((unsigned)((ngenomes + 255) / 256)), dim3(256), 0, s, first, count, ngenomes, seg_end);
    return rocprim::segmented_radix_sort_keys(tmp, tmp_bytes, comp, sorted, total, (unsigned)ngenomes, first, (const unsigned *)seg_end, 0u,
                                              (unsigned)mash_value_bits(k), s);
}

void launch_mash_unique(const uint64_t *sorted, const unsigned *first, const unsigned *count, int ngenomes, int s, uint64_t *sketch, int *len, hipStream_t st) {
    if (ngenomes <= 0) return;
    hipLaunchKernelGGL(k_mash_unique, dim3((unsigned)ngenomes), dim3(256), 0, st, sorted, first, count, s, sketch, len);
}

void launch_mash_pairs(const uint64_t *sketch, const int *len, const int *rows, int nrows, const int *cols, int ncols, int s, int2 *out, hipStream_t st) {
    if (nrows <= 0 || ncols <= 0) return;
    hipLaunchKernelGGL(k_mash_pairs, dim3((unsigned)ncols, (unsigned)nrows), dim3(MASH_CHUNK), 0, st, sketch, len, rows, cols, ncols, s, out);
}

}  // namespace pml
