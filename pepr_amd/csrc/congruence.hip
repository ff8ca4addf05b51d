// congruence.hip -- the reference's `-congruence_filter` (PhylogenomicPipeline2.filterForCongruence, :429-511) on the device.
//
// Every alignment column becomes bipartitions ("splits") of the n taxa of the concatenation; the non-trivial splits are counted
// over all columns, the most frequent ones are kept (the host picks them), and every gene is charged, for each of its distinct
// splits, the column counts of the kept splits that conflict with it.  Everything is integer work on sets of n <= 512 bits:
// a split is W = 1, 2, 4 or 8 64-bit words (template parameter), taxon i = bit i & 63 of word i >> 6.
//
// k_colsplits      workgroup = CG_COLS columns of one gene staged in LDS (rows are contiguous, so the 16-byte loads are
//                  coalesced), thread = one column.  The thread keeps a 256-bit mask of the bytes it has seen and the number of
//                  taxa that show neither '-' nor '?'.  The count pass stores the column's number of splits: its number of
//                  classes, less one when two classes cover all n taxa (they normalise to the same split).  The write pass
//                  rescans the staged column once per class (ascending byte), builds the class in registers (the rows come in
//                  ascending union index, so word w is finished before word w + 1 starts), normalises it (complement over ALL
//                  n taxa, the smaller side kept, on a tie the side with taxon 0) and stores W words, the gene and the column.
// k_split_intern   thread = one record.  Open addressing, one 32-bit atomicCAS per probe: a slot holds the index of the first
//                  record with its key.  A taken slot is compared against the OWNER's record, which the previous launch wrote.
//                  The record leaves with the owner's index as its split id and, when it has at least 2 members, adds 1 to the
//                  owner's column count.
// k_split_gather   the kept splits' words, contiguous.
// k_splitcost      thread = one distinct split, in registers; the kept splits stream through LDS in tiles of CG_KTILE (their
//                  number has no bound); every lane reads the same entry at the same time (broadcast).  b and k conflict when
//                  b & k is non-empty and differs from both.  64-bit sums.
// k_genecost       thread = one record; a second table keyed by gene << 32 | split id, one 64-bit atomicCAS per probe; the
//                  thread that claims a slot adds the split's cost to its gene's sum and 1 to its gene's distinct count
//                  (summed per wavefront first when the wavefront's records are of one gene, which they nearly always are).
//
// No thread waits for another thread's write: a slot is only compared with data an earlier launch finished, the CAS word
// aside.  Every probe loop is bounded by the table's capacity; one that runs out sets *err.  Every result is an integer sum
// or a set: nothing depends on the order of the atomics.  No kernel allocates.
#include "kernels.h"

namespace pml {

static_assert(CG_COLS == 64 && CG_MAX_TAXA == 512, "one wavefront per tile of columns; 8 words hold every taxon");
constexpr int CG_ROW = CG_COLS + 16;          // LDS stride of a staged row: 20 words, so 8 consecutive rows start in different banks

__device__ __forceinline__ unsigned long long cg_hash(const unsigned long long *a, int W) {
    unsigned long long h = 0x9E3779B97F4A7C15ull;
    for (int w = 0; w < W; ++w) h = mix64(h ^ a[w]) + 0x9E3779B97F4A7C15ull * (unsigned)(w + 1);
    return h;
}

template <int W>
__global__ __launch_bounds__(CG_COLS) void k_colsplits(const CgGene *__restrict__ genes, const int *__restrict__ tile_gene, const int *__restrict__ tile_first,
                                                       int n, int *__restrict__ nsplit, const long long *__restrict__ rec_off,
                                                       unsigned long long *__restrict__ rec, int *__restrict__ rec_gene, long long *__restrict__ rec_col) {
    extern __shared__ __attribute__((aligned(16))) uint8_t cg_lds[];
    const int gi = tile_gene[blockIdx.x];
    const CgGene g = genes[gi];
    const int c0 = ((int)blockIdx.x - tile_first[gi]) * CG_COLS;
    uint8_t *rows = cg_lds;                                            // [g.ntax][CG_ROW]
    uint16_t *map = (uint16_t *)(cg_lds + (size_t)g.ntax * CG_ROW);    // [g.ntax]; g.ntax * CG_ROW is a multiple of 16
    const int tid = threadIdx.x;
    for (int v = tid; v < g.ntax * (CG_COLS / 16); v += CG_COLS) {
        const int row = v / (CG_COLS / 16), q = v % (CG_COLS / 16);
        // c0 + q * 16 < ncols <= ld, and ld and c0 are multiples of 16: the 16 bytes lie inside the row
        if (c0 + q * 16 < g.ncols) *(uint4 *)&rows[row * CG_ROW + q * 16] = *(const uint4 *)(g.bytes + (size_t)row * g.ld + c0 + q * 16);
    }
    for (int r = tid; r < g.ntax; r += CG_COLS) map[r] = g.map[r];
    __syncthreads();
    const int c = c0 + tid;
    if (c >= g.ncols) return;                                          // no barrier follows
    unsigned long long seen[4] = {0, 0, 0, 0};
    int shown = 0;                                                     // taxa with a byte other than '-' and '?'
    for (int r = 0; r < g.ntax; ++r) {
        const unsigned b = rows[r * CG_ROW + tid];
        const unsigned long long bit = 1ull << (b & 63);
        const unsigned w = b >> 6;
        seen[0] |= w == 0 ? bit : 0; seen[1] |= w == 1 ? bit : 0; seen[2] |= w == 2 ? bit : 0; seen[3] |= w == 3 ? bit : 0;
        shown += b != '-' && b != '?';
    }
    seen[0] &= ~((1ull << '-') | (1ull << '?'));                       // both below 64
    const int classes = __popcll(seen[0]) + __popcll(seen[1]) + __popcll(seen[2]) + __popcll(seen[3]);
    const int count = classes == 2 && shown == n ? 1 : classes;        // two classes that cover all n taxa are one split
    const long long col = g.col_base + c;
    if (!rec) { nsplit[col] = count; return; }
    long long at = rec_off[col];
    int left = count;
#pragma unroll
    for (int sw = 0; sw < 4; ++sw) {
        unsigned long long m = seen[sw];
        while (m && left > 0) {
            const unsigned byte = (unsigned)(sw * 64 + __ffsll((long long)m) - 1);
            m &= m - 1;
            unsigned long long a[W];
            int r = 0, members = 0;
#pragma unroll
            for (int w = 0; w < W; ++w) {
                unsigned long long word = 0;
                for (; r < g.ntax && (map[r] >> 6) == w; ++r) word |= rows[r * CG_ROW + tid] == byte ? 1ull << (map[r] & 63) : 0;
                a[w] = word; members += __popcll(word);
            }
            if (2 * members > n || (2 * members == n && !(a[0] & 1))) {
#pragma unroll
                for (int w = 0; w < W; ++w) {
                    const int bits = n - w * 64;                       // taxa in this word and above
                    a[w] = ~a[w] & (bits >= 64 ? ~0ull : bits > 0 ? (1ull << bits) - 1 : 0);
                }
            }
#pragma unroll
            for (int w = 0; w < W; ++w) rec[at * W + w] = a[w];
            rec_gene[at] = gi; rec_col[at] = col;
            ++at; --left;
        }
    }
}

template <int W>
__global__ __launch_bounds__(256) void k_split_intern(const unsigned long long *__restrict__ rec, long long nrec, int *slot, unsigned long long cap,
                                                      unsigned long long hash_mask, int *__restrict__ split_id, int *count, int *err) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= nrec) return;
    unsigned long long a[W];
    int members = 0;
#pragma unroll
    for (int w = 0; w < W; ++w) { a[w] = rec[r * W + w]; members += __popcll(a[w]); }
    unsigned long long s = (cg_hash(a, W) & hash_mask) & (cap - 1);
    int owner = -1;
    for (unsigned long long probe = 0; probe < cap; ++probe, s = (s + 1) & (cap - 1)) {
        int cur = slot[s];                                             // a plain look first: most probes hit a taken slot
        if (cur < 0) cur = atomicCAS(&slot[s], -1, (int)r);
        if (cur < 0) { owner = (int)r; break; }                        // claimed
        bool same = true;
#pragma unroll
        for (int w = 0; w < W; ++w) same = same && rec[(long long)cur * W + w] == a[w];       // the owner's record: written by the launch before
        if (same) { owner = cur; break; }
    }
    if (owner < 0) { atomicOr(err, 1); split_id[r] = (int)r; return; }
    split_id[r] = owner;
    if (members >= 2) atomicAdd(&count[owner], 1);
}

template <int W>
__global__ __launch_bounds__(256) void k_split_gather(const unsigned long long *__restrict__ rec, const int *__restrict__ idx, long long nidx,
                                                      unsigned long long *__restrict__ out) {
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j >= nidx) return;
    const long long src = idx[j];
#pragma unroll
    for (int w = 0; w < W; ++w) out[j * W + w] = rec[src * W + w];
}

template <int W>
__global__ __launch_bounds__(256) void k_splitcost(const unsigned long long *__restrict__ rec, const int *__restrict__ dist, long long ndist,
                                                   const unsigned long long *__restrict__ kwords, const int *__restrict__ kcount, long long nkept,
                                                   long long *__restrict__ cost_d, long long *__restrict__ cost_rec) {
    __shared__ unsigned long long tw[CG_KTILE * W];
    __shared__ int tc[CG_KTILE];
    const long long d = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool active = d < ndist;
    const long long owner = active ? dist[d] : 0;
    unsigned long long b[W];
#pragma unroll
    for (int w = 0; w < W; ++w) b[w] = active ? rec[owner * W + w] : 0;
    long long cost = 0;
    for (long long k0 = 0; k0 < nkept; k0 += CG_KTILE) {
        const int len = (int)(nkept - k0 < CG_KTILE ? nkept - k0 : CG_KTILE);
        for (int v = threadIdx.x; v < len * W; v += 256) tw[v] = kwords[k0 * W + v];
        for (int v = threadIdx.x; v < len; v += 256) tc[v] = kcount[k0 + v];
        __syncthreads();
        for (int j = 0; j < len; ++j) {
            unsigned long long any = 0, nb = 0, nk = 0;
#pragma unroll
            for (int w = 0; w < W; ++w) {
                const unsigned long long k = tw[j * W + w], x = b[w] & k;
                any |= x; nb |= x ^ b[w]; nk |= x ^ k;
            }
            cost += any && nb && nk ? tc[j] : 0;
        }
        __syncthreads();
    }
    if (active) { cost_d[d] = cost; cost_rec[owner] = cost; }
}

__global__ __launch_bounds__(256) void k_genecost(const int *__restrict__ rec_gene, const int *__restrict__ split_id, long long nrec,
                                                  const long long *__restrict__ cost_rec, unsigned long long *keys, unsigned long long cap,
                                                  unsigned long long hash_mask, long long *cost_sum, int *ndistinct, int *err) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool active = r < nrec;
    const int gene = active ? rec_gene[r] : -1;
    bool claimed = false;
    int id = 0;
    if (active) {
        id = split_id[r];
        const unsigned long long key = ((unsigned long long)(unsigned)gene << 32) | (unsigned)id;
        unsigned long long s = (mix64(key) & hash_mask) & (cap - 1);
        bool done = false;
        for (unsigned long long probe = 0; probe < cap && !done; ++probe, s = (s + 1) & (cap - 1)) {
            unsigned long long cur = keys[s];
            if (cur == ~0ull) { cur = atomicCAS(&keys[s], ~0ull, key); claimed = cur == ~0ull; }
            done = claimed || cur == key;
        }
        if (!done) atomicOr(err, 1);
    }
    long long add = claimed ? cost_rec[id] : 0;
    int one = claimed ? 1 : 0;
    // the records of a gene are consecutive: a wavefront of one gene sums first and issues one pair of atomics
    const int g0 = __shfl(gene, 0);
    if (__all(gene == g0 || !active)) {
        for (int off = 32; off > 0; off >>= 1) { add += __shfl_xor(add, off); one += __shfl_xor(one, off); }
        if ((threadIdx.x & 63) == 0 && one) { atomicAdd((unsigned long long *)&cost_sum[g0], (unsigned long long)add); atomicAdd(&ndistinct[g0], one); }
    } else if (claimed) {
        atomicAdd((unsigned long long *)&cost_sum[gene], (unsigned long long)add); atomicAdd(&ndistinct[gene], 1);
    }
}

#define CG_DISPATCH(W, CALL)                                                                                          \
    switch (W) { case 1: { constexpr int W_ = 1; CALL; break; } case 2: { constexpr int W_ = 2; CALL; break; }        \
                 case 4: { constexpr int W_ = 4; CALL; break; } default: { constexpr int W_ = 8; CALL; break; } }

void launch_colsplits(const CgGene *genes, const int *tile_gene, const int *tile_first, int ntiles, int max_ntax, int n, int *nsplit,
                      const long long *rec_off, unsigned long long *rec, int *rec_gene, long long *rec_col, hipStream_t s) {
    if (ntiles <= 0) return;
    const size_t lds = (size_t)max_ntax * CG_ROW + (size_t)max_ntax * sizeof(uint16_t);     // at most 512 * 82 = 41984 bytes
    CG_DISPATCH(cg_words(n), hipLaunchKernelGGL(k_colsplits<W_>, dim3((unsigned)ntiles), dim3(CG_COLS), lds, s, genes, tile_gene, tile_first, n, nsplit,
                                                rec_off, rec, rec_gene, rec_col));
}

void launch_split_intern(const unsigned long long *rec, long long nrec, int W, int *slot, unsigned long long cap, unsigned long long hash_mask,
                         int *split_id, int *count, int *err, hipStream_t s) {
    if (nrec <= 0) return;
    CG_DISPATCH(W, hipLaunchKernelGGL(k_split_intern<W_>, dim3((unsigned)((nrec + 255) / 256)), dim3(256), 0, s, rec, nrec, slot, cap, hash_mask, split_id, count, err));
}

void launch_split_gather(const unsigned long long *rec, const int *idx, long long nidx, int W, unsigned long long *out, hipStream_t s) {
    if (nidx <= 0) return;
    CG_DISPATCH(W, hipLaunchKernelGGL(k_split_gather<W_>, dim3((unsigned)((nidx + 255) / 256)), dim3(256), 0, s, rec, idx, nidx, out));
}

void launch_splitcost(const unsigned long long *rec, const int *dist, long long ndist, int W, const unsigned long long *kwords, const int *kcount,
                      long long nkept, long long *cost_d, long long *cost_rec, hipStream_t s) {
    if (ndist <= 0) return;
    CG_DISPATCH(W, hipLaunchKernelGGL(k_splitcost<W_>, dim3((unsigned)((ndist + 255) / 256)), dim3(256), 0, s, rec, dist, ndist, kwords, kcount, nkept, cost_d, cost_rec));
}

void launch_genecost(const int *rec_gene, const int *split_id, long long nrec, const long long *cost_rec, unsigned long long *keys,
                     unsigned long long cap, unsigned long long hash_mask, long long *cost_sum, int *ndistinct, int *err, hipStream_t s) {
    if (nrec <= 0) return;
    hipLaunchKernelGGL(k_genecost, dim3((unsigned)((nrec + 255) / 256)), dim3(256), 0, s, rec_gene, split_id, nrec, cost_rec, keys, cap, hash_mask, cost_sum, ndistinct, err);
}

}  // namespace pml
