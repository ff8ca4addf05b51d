// treecmp.hip -- TreeComparison's `-rf` and `-tree_dist` legs (compareAllvsAll, TreeComparison.java:267-288) for a whole set of
// trees on the device.  The host (treecmp.cpp) turns every tree into split records in the Java's branch order; here they are
// interned, sorted per tree, and every scheduled pair of trees is compared by one lane.
//
// k_split_intern   congruence.hip's kernel as it is: every record leaves with the index of SOME record of its split.
// k_tree_first     first[owner] = min over the records of that owner of their index; then id = first[owner]: the id of a
//                  split is the index of its first occurrence in the call, whichever thread won the table slot.
// k_tree_sort      workgroup = one tree.  Its (id, record index) pairs are sorted in LDS (bitonic, 64-bit keys id << 32 | index,
//                  so for equal ids the highest index comes last) and written to sid / sidx; a record that is the last of its
//                  id in the tree gets TC_LAST: that record is the one HashMap.put leaves in tree2SetsToBranches
//                  (TreeComparison.java:631-636) and the representative when distinct splits are counted.
// k_tree_sums      thread = one tree: its two sums of squares (normalised and raw lengths, ascending branch index, one
//                  thread's registers) and its numbers of distinct splits (all, non-trivial).
// k_tree_pairs     workgroup = one row tree i and TC_COLS column trees; tree i's records and its sorted ids are staged in LDS;
//                  lane = one column tree j >= i.  Loop 1 walks i's records in branch order (every lane reads the same LDS
//                  word: a broadcast) and binary-searches j's sorted ids in global memory for the counterpart: 4 bytes per
//                  probe whatever n is.  Loop 2 walks j's branches in j's order and binary-searches i's sorted ids in LDS.
//                  The lane carries the running sums r of getBranchDistance (:691-694, :737-743) and of
//                  getDiscrepantBranchDistance (:783-806) from the first term to the last; floating-point contraction is off
//                  for this file, so no multiply-add is fused; the square roots and the division are the host's.
//
// Bounds: a tree's records are off[t] .. off[t] + cnt[t] - 1 of the compact arrays, cnt[t] <= maxrec (the LDS size); a search
// never leaves [0, cnt); trees beyond T, below the diagonal or outside the window return after the staging barrier.
#include "kernels.h"

#pragma clang fp contract(off)

namespace pml {

// sum + x * x as the Java rounds it: a rounded multiply, then a rounded add.  The file is compiled with contraction off (the
// pragma above): the runtime's __dmul_rn / __dadd_rn are inline functions of a header compiled with contraction ON, so a
// multiply and an add that come from them DO fuse once inlined -- plain operators under the pragma do not
__device__ __forceinline__ double tc_acc(double sum, double x) {
    const double sq = x * x;
    return sum + sq;
}

__global__ __launch_bounds__(256) void k_tree_first(const int *__restrict__ owner, long long nrec, int *first) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r < nrec) atomicMin(&first[owner[r]], (int)r);
}

__global__ __launch_bounds__(256) void k_tree_first_apply(int *id, long long nrec, const int *__restrict__ first) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r < nrec) id[r] = first[id[r]];
}

__global__ __launch_bounds__(256) void k_tree_sort(TcTrees t) {
    __shared__ unsigned long long key[TC_SORT];
    const int tree = blockIdx.x;
    const int off = t.off[tree], cnt = min(t.cnt[tree], TC_SORT);
    for (int v = threadIdx.x; v < TC_SORT; v += 256) key[v] = v < cnt ? ((unsigned long long)(unsigned)t.id[off + v] << 32) | (unsigned)v : ~0ull;
    __syncthreads();
    for (int k = 2; k <= TC_SORT; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int v = threadIdx.x; v < TC_SORT; v += 256) {
                const int w = v ^ j;
                if (w > v) {
                    const unsigned long long a = key[v], b = key[w];
                    if (((v & k) == 0) == (a > b)) { key[v] = b; key[w] = a; }
                }
            }
            __syncthreads();
        }
    for (int v = threadIdx.x; v < cnt; v += 256) {
        const int id = (int)(key[v] >> 32), idx = (int)(key[v] & 0xFFFFFFFFu);
        t.sid[off + v] = id; t.sidx[off + v] = idx;
        if (v + 1 == cnt || (int)(key[v + 1] >> 32) != id) t.flags[off + idx] |= TC_LAST;      // idx < cnt: one writer per record
    }
}

__global__ __launch_bounds__(256) void k_tree_sums(TcTrees t, double *__restrict__ ss /* [T][2] */, int *__restrict__ distinct /* [T][2] */) {
    const int tree = blockIdx.x * 256 + threadIdx.x;
    if (tree >= t.T) return;
    const int off = t.off[tree], nreal = min(t.nreal[tree], t.cnt[tree]);
    double sn = 0, sr = 0; int da = 0, dn = 0;
    for (int b = 0; b < nreal; ++b) {
        const double ln = t.ln[off + b], lr = t.lr[off + b];
        sn = tc_acc(sn, ln);
        sr = tc_acc(sr, lr);
        const int f = t.flags[off + b];
        if (f & TC_LAST) { ++da; dn += !(f & TC_TRIVIAL); }
    }
    ss[2 * tree] = sn; ss[2 * tree + 1] = sr; distinct[2 * tree] = da; distinct[2 * tree + 1] = dn;
}

// the index of the LAST entry of sid[0 .. n) equal to key, or -1
__device__ __forceinline__ int tc_find(const int *sid, int n, int key) {
    int lo = 0, hi = n;
    while (lo < hi) { const int m = (lo + hi) >> 1; if (sid[m] <= key) lo = m + 1; else hi = m; }
    return lo > 0 && sid[lo - 1] == key ? lo - 1 : -1;
}

__global__ __launch_bounds__(TC_COLS) void k_tree_pairs(TcTrees t, int i0, int nrows, int window, int maxrec, int4 *__restrict__ counts, double2 *__restrict__ sums) {
    extern __shared__ __attribute__((aligned(16))) unsigned char tc_lds[];
    const int row = blockIdx.y;
    const int i = i0 + row;
    if (row >= nrows || i >= t.T) return;                                          // uniform over the workgroup
    const int jlast = min((int)blockIdx.x * TC_COLS + TC_COLS - 1, t.T - 1);
    if (jlast < i || (window > 0 && (int)blockIdx.x * TC_COLS - i > window)) return;      // uniform: nothing to do in this tile
    double *l_ln = (double *)tc_lds, *l_lr = l_ln + maxrec;
    int *l_id = (int *)(l_lr + maxrec), *l_fl = l_id + maxrec, *l_sid = l_fl + maxrec, *l_sidx = l_sid + maxrec;
    const int offi = t.off[i], cnti = min(t.cnt[i], maxrec);
    for (int v = threadIdx.x; v < cnti; v += TC_COLS) {
        l_ln[v] = t.ln[offi + v]; l_lr[v] = t.lr[offi + v]; l_id[v] = t.id[offi + v]; l_fl[v] = t.flags[offi + v];
        l_sid[v] = t.sid[offi + v]; l_sidx[v] = t.sidx[offi + v];
    }
    __syncthreads();
    const int j = (int)blockIdx.x * TC_COLS + threadIdx.x;
    if (j >= t.T || j < i || (window > 0 && j - i > window)) return;               // no barrier follows
    const int offj = t.off[j], cntj = t.cnt[j], nrealj = min(t.nreal[j], cntj);
    const int *sidj = t.sid + offj, *sidxj = t.sidx + offj, *flj = t.flags + offj, *idj = t.id + offj;
    const double *lnj = t.ln + offj, *lrj = t.lr + offj;
    double rb = 0, rd = 0;
    int s_all = 0, s_nt = 0, s_res = 0;
    for (int b = 0; b < cnti; ++b) {
        const int f = l_fl[b];
        const int e = tc_find(sidj, cntj, l_id[b]);
        const int c = e >= 0 ? sidxj[e] : -1;                                      // c < cntj: k_tree_sort wrote indices below cnt
        const bool creal = c >= 0 && c < cntj && (flj[c] & TC_REAL);
        if (f & TC_REAL) {
            rb = tc_acc(rb, l_ln[b] - (creal ? lnj[c] : 0.0));
            if (!creal) rd = tc_acc(rd, l_lr[b] - 0.0);
            if ((f & TC_LAST) && creal) { ++s_all; s_nt += !(f & TC_TRIVIAL); }
        }
        if ((f & TC_LAST) && !(f & TC_TRIVIAL) && c >= 0) ++s_res;
    }
    for (int k = 0; k < nrealj; ++k) {
        bool checked = false;
        if (flj[k] & TC_LAST) {
            const int e = tc_find(l_sid, cnti, idj[k]);
            if (e >= 0) { const int bi = l_sidx[e]; checked = bi >= 0 && bi < cnti && (l_fl[bi] & TC_REAL); }
        }
        if (!checked) {
            rb = tc_acc(rb, lnj[k]);
            rd = tc_acc(rd, lrj[k]);
        }
    }
    const size_t at = (size_t)row * t.T + j;
    counts[at] = make_int4(s_all, s_nt, s_res, 0);
    sums[at] = make_double2(rb, rd);
}

void launch_tree_first(int *id, long long nrec, int *first, hipStream_t s) {
    if (nrec <= 0) return;
    const unsigned blocks = (unsigned)((nrec + 255) / 256);
    hipLaunchKernelGGL(k_tree_first, dim3(blocks), dim3(256), 0, s, id, nrec, first);
    hipLaunchKernelGGL(k_tree_first_apply, dim3(blocks), dim3(256), 0, s, id, nrec, first);
}

void launch_tree_sort(const TcTrees &t, double *ss, int *distinct, hipStream_t s) {
    if (t.T <= 0) return;
    hipLaunchKernelGGL(k_tree_sort, dim3((unsigned)t.T), dim3(256), 0, s, t);
    hipLaunchKernelGGL(k_tree_sums, dim3((unsigned)((t.T + 255) / 256)), dim3(256), 0, s, t, ss, distinct);
}

size_t tree_pairs_lds(int maxrec) { return (size_t)maxrec * (2 * sizeof(double) + 4 * sizeof(int)); }

void launch_tree_pairs(const TcTrees &t, int i0, int nrows, int window, int maxrec, int4 *counts, double2 *sums, hipStream_t s) {
    if (nrows <= 0 || t.T <= 0) return;
    hipLaunchKernelGGL(k_tree_pairs, dim3((unsigned)((t.T + TC_COLS - 1) / TC_COLS), (unsigned)nrows), dim3(TC_COLS), tree_pairs_lds(maxrec), s, t, i0, nrows, window,
                       maxrec, counts, sums);
}

}  // namespace pml
