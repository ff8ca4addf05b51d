// mcl.hip -- Markov clustering of the hit graph's components (the rule: include/peprml.h "Homolog groups"; layout and budgets:
// DESIGN.md section 4).  All arithmetic is f64; every expansion C = A A runs on v_mfma_f64_16x16x4_f64 (lane l feeds
// A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15], and receives D[row = (l >> 4) + 4 reg][col = l & 15], reg = 0..3).
// A matrix is column major.  Three classes:
//   packed  n <= 16: k_mcl_lds<true>, four components per workgroup, one wavefront each, two 16 x 18 buffers per component in LDS
//   LDS     n <= 96: k_mcl_lds<false>, one workgroup per component, two 96 x 98 buffers (150.5 KB) in LDS
//   HBM     larger: k_mcl_expand (64 x 64 tiles of C, LDS-staged panels 16 deep) and k_mcl_inflate (a workgroup per column) per
//           iteration, k_mcl_flag's one flag per component read by the host between iterations, k_mcl_read at the end
// The two LDS kernels run the whole iteration loop in ONE launch, bounded by max_iter; their barriers are workgroup barriers that
// every wavefront reaches the same number of times (a component that has converged idles until the workgroup's last one has).
// No kernel waits on another workgroup.  Reductions are shuffle butterflies and fixed-order loops: the same bits every run.
#include "kernels.h"

namespace pml {

typedef double v4d __attribute__((ext_vector_type(4)));

namespace {

__device__ __forceinline__ double shfl_xor_d(double v, int m) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __shfl_xor(lo, m); hi = __shfl_xor(hi, m);
    return __hiloint2double(hi, lo);
}
// over the 16 lanes that share lane >> 4; every lane receives the same bits (a + b == b + a)
__device__ __forceinline__ double sum16(double v) { for (int m = 8; m >= 1; m >>= 1) v += shfl_xor_d(v, m); return v; }
__device__ __forceinline__ double max16(double v) { for (int m = 8; m >= 1; m >>= 1) v = fmax(v, shfl_xor_d(v, m)); return v; }
__device__ __forceinline__ double sum64(double v) { for (int m = 32; m >= 1; m >>= 1) v += shfl_xor_d(v, m); return v; }
__device__ __forceinline__ double max64(double v) { for (int m = 32; m >= 1; m >>= 1) v = fmax(v, shfl_xor_d(v, m)); return v; }
// the better of two (value, row) candidates: a row < 0 is none; the larger value, the lower row of equals
__device__ __forceinline__ void better(double &v, int &i, double v2, int i2) {
    if (i2 >= 0 && (i < 0 || v2 > v || (v2 == v && i2 < i))) { v = v2; i = i2; }
}

}  // namespace

// the start matrix of every component of a sub-batch from the CSR: thread = one column (the pool is zeroed by the caller)
__global__ void __launch_bounds__(64) k_mcl_fill(const MclComp *comps, const long long *ptr, const int *row, const double *val, double *pool) {
    const MclComp c = comps[blockIdx.y];
    const int j = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (j >= c.n) return;
    const long long k0 = ptr[c.col0 + j], k1 = ptr[c.col0 + j + 1];
    double mx = 0, sum = 0;
    for (long long k = k0; k < k1; ++k) { mx = fmax(mx, val[k]); sum += val[k]; }
    const double loop = mx > 0 ? mx : 1.0;
    sum += loop;
    double *col = pool + c.mat + (size_t)j * c.npad;
    for (long long k = k0; k < k1; ++k) col[row[k]] = val[k] / sum;
    col[j] = loop / sum;
}

// The LDS classes.  PACKED: team = one wavefront, component blockIdx.x * 4 + wave, NP = 16.  Otherwise team = the workgroup.
// A component's matrix is n x n in HBM (column stride n); write_back puts the final matrix back there (test door).
template <bool PACKED>
__global__ void __launch_bounds__(MCL_THREADS) k_mcl_lds(const MclComp *comps, int ncomps, double *pool, MclRun run, int *best, unsigned *mask, int *iters,
                                                         double *chaos_out, int write_back) {
    constexpr int TEAMS = PACKED ? 4 : 1, NPMAX = PACKED ? MCL_PACKED_MAX : MCL_LDS_MAX, LD = NPMAX + 2, R = NPMAX / 16;
    constexpr int TEAM_THREADS = MCL_THREADS / TEAMS, TEAM_WAVES = TEAM_THREADS / 64, GROUPS = TEAM_THREADS / 16;
    extern __shared__ double mcl_dyn[];                      // TEAMS x 2 buffers of NPMAX x LD
    __shared__ double s_chaos[TEAMS][NPMAX];
    __shared__ int s_att[TEAMS][NPMAX];
    __shared__ int s_act[TEAMS];
    __shared__ double s_last[TEAMS];
    const int tid = (int)threadIdx.x, team = PACKED ? tid >> 6 : 0, tt = tid & (TEAM_THREADS - 1), wave = tt >> 6, lane = tid & 63;
    const int q = lane >> 4, r16 = lane & 15, g = tt >> 4;
    const int ci = (int)blockIdx.x * TEAMS + team;
    const bool have = ci < ncomps;
    MclComp c; c.mat = 0; c.n = 0; c.npad = 0; c.col0 = 0; c.pad = 0; c.mask_off = 0;
    if (have) c = comps[ci];
    const int n = c.n, NP = (n + 15) & ~15, nt = NP >> 4;
    double *const base = mcl_dyn + (size_t)team * 2 * NPMAX * LD;     // buffer b of the team at base + b * NPMAX * LD
    for (int i = tt; i < 2 * NPMAX * LD; i += TEAM_THREADS) base[i] = 0.0;
    __syncthreads();
    {
        const double *src = pool + c.mat;
        for (int i = tt; i < n * n; i += TEAM_THREADS) base[(i / n) * LD + (i % n)] = src[i];
    }
    if (tt == 0) { s_act[team] = have && n > 0 ? 1 : 0; s_last[team] = 0.0; }
    __syncthreads();
    int cur = 0, done = 0;
    const double thr = 1.0 / run.prune_inverse;
    for (int it = 0; it < run.max_iter; ++it) {
        const bool act = s_act[team] != 0;
        bool any = false;
        for (int t = 0; t < TEAMS; ++t) any = any || s_act[t] != 0;
        if (!any) break;                                     // uniform: read behind the barrier that ended the last round
        const double *src = base + cur * NPMAX * LD;
        double *dst = base + (cur ^ 1) * NPMAX * LD;
        if (act) {                                           // expansion: 16 x 16 tiles of dst, NP / 4 chained MFMAs each
            for (int t = wave; t < nt * nt; t += TEAM_WAVES) {
                const int ti = t % nt, tj = t / nt;
                v4d acc = {0.0, 0.0, 0.0, 0.0};
                for (int k = 0; k < NP; k += 4) {
                    const double a = src[(k + q) * LD + ti * 16 + r16];
                    const double b = src[(tj * 16 + r16) * LD + k + q];
                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
                }
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) dst[(tj * 16 + r16) * LD + ti * 16 + q + 4 * reg] = acc[reg];
            }
        }
        __syncthreads();
        if (act) {                                           // the column work: 16 lanes per column, R rows per lane
            for (int j0 = 0; j0 < n; j0 += GROUPS) {
                const int j = j0 + g;
                const bool ok = j < n;
                double *col = dst + (ok ? j : 0) * LD;
                double v[R], s = 0;
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const int i = r16 + 16 * r;
                    double x = ok && i < n ? col[i] : 0.0;
                    if (x < thr) x = 0.0;
                    v[r] = x; s += x;
                }
                s = sum16(s);
                double mx = 0, sq = 0;
#pragma unroll
                for (int r = 0; r < R; ++r) { v[r] = s > 0 ? v[r] / s : 0.0; mx = fmax(mx, v[r]); sq += v[r] * v[r]; }
                mx = max16(mx); sq = sum16(sq);
                double s2 = 0;
#pragma unroll
                for (int r = 0; r < R; ++r) { v[r] = v[r] > 0 ? pow(v[r], run.inflation) : 0.0; s2 += v[r]; }
                s2 = sum16(s2);
                if (ok) {
#pragma unroll
                    for (int r = 0; r < R; ++r) { const int i = r16 + 16 * r; if (i < n) col[i] = s2 > 0 ? v[r] / s2 : 0.0; }
                    if (r16 == 0) s_chaos[team][j] = mx - sq;
                }
            }
            cur ^= 1;
            done = it + 1;
        }
        __syncthreads();
        if (act && tt == 0) {                                // chaos in a fixed order
            double ch = s_chaos[team][0];
            for (int j = 1; j < n; ++j) ch = fmax(ch, s_chaos[team][j]);
            s_last[team] = ch;
            if (ch < run.chaos_eps) s_act[team] = 0;
        }
        __syncthreads();
    }
    // the reading: attractors, every column's best attractor row, the attractor columns' masks
    const double *M = base + cur * NPMAX * LD;
    for (int i = tt; i < n; i += TEAM_THREADS) s_att[team][i] = M[i * LD + i] > 0 ? 1 : 0;
    __syncthreads();
    const int W = (n + 31) >> 5;
    for (int j0 = 0; j0 < n; j0 += GROUPS) {
        const int j = j0 + g;
        const bool ok = j < n;
        const double *col = M + (ok ? j : 0) * LD;
        double bv = 0; int bi = -1;
        unsigned w[(NPMAX + 31) / 32];
#pragma unroll
        for (int k = 0; k < (NPMAX + 31) / 32; ++k) w[k] = 0;
        const bool att_j = ok && s_att[team][j] != 0;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int i = r16 + 16 * r;
            if (ok && i < n && s_att[team][i]) {
                const double x = col[i];
                better(bv, bi, x, i);
                if (att_j && x > 0) w[(16 * r) >> 5] |= 1u << (i & 31);       // r16 < 16: the word depends on r alone
            }
        }
        for (int m = 8; m >= 1; m >>= 1) {
            const double v2 = shfl_xor_d(bv, m); const int i2 = __shfl_xor(bi, m);
            better(bv, bi, v2, i2);
#pragma unroll
            for (int k = 0; k < (NPMAX + 31) / 32; ++k) w[k] |= (unsigned)__shfl_xor((int)w[k], m);
        }
        if (ok && r16 == 0) {
            best[c.col0 + j] = bi;
#pragma unroll
            for (int k = 0; k < (NPMAX + 31) / 32; ++k) if (k < W) mask[c.mask_off + (size_t)j * W + k] = w[k];
        }
    }
    if (have && tt == 0) { iters[ci] = done; chaos_out[ci] = s_last[team]; }
    if (write_back && have) {
        double *out = pool + c.mat;
        for (int i = tt; i < n * n; i += TEAM_THREADS) out[i] = M[(i / n) * LD + (i % n)];
    }
}

// HBM class: C = A A for the active components, a 64 x 64 tile of C per workgroup.  A matrix is npad x npad (npad a multiple of
// 64, the padding zero), buffer B behind buffer A; parity 0 reads A and writes B
__global__ void __launch_bounds__(MCL_THREADS) k_mcl_expand(const MclComp *comps, const int *active, double *pool, int parity) {
    const MclComp c = comps[active[blockIdx.z]];
    const int T = c.npad / MCL_TILE;
    if ((int)blockIdx.x >= T || (int)blockIdx.y >= T) return;
    const size_t ld = (size_t)c.npad;
    const double *A = pool + c.mat + (parity ? ld * ld : 0);
    double *C = pool + c.mat + (parity ? 0 : ld * ld);
    const int row0 = (int)blockIdx.x * MCL_TILE, col0 = (int)blockIdx.y * MCL_TILE;
    __shared__ double sA[MCL_KSTEP][MCL_TILE + 16];          // sA[k][i] = A[row0 + i][k0 + k]
    __shared__ double sB[MCL_TILE][MCL_KSTEP + 2];           // sB[j][k] = A[k0 + k][col0 + j]
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63, q = lane >> 4, r16 = lane & 15;
    v4d acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = v4d{0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < c.npad; k0 += MCL_KSTEP) {
#pragma unroll
        for (int e = 0; e < MCL_KSTEP * MCL_TILE / MCL_THREADS; ++e) {
            const int idx = tid + MCL_THREADS * e;
            sA[idx >> 6][idx & 63] = A[(size_t)(k0 + (idx >> 6)) * ld + row0 + (idx & 63)];
            sB[idx >> 4][idx & 15] = A[(size_t)(col0 + (idx >> 4)) * ld + k0 + (idx & 15)];
        }
        __syncthreads();
#pragma unroll
        for (int k4 = 0; k4 < MCL_KSTEP; k4 += 4) {
            const double b = sB[16 * wave + r16][k4 + q];
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(sA[k4 + q][16 * t + r16], b, acc[t], 0, 0, 0);
        }
        __syncthreads();
    }
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) C[(size_t)(col0 + 16 * wave + r16) * ld + row0 + 16 * t + q + 4 * reg] = acc[t][reg];
}

namespace {
// block reductions of 256 threads: butterflies inside the wavefronts, then the four partial results in order
__device__ __forceinline__ double block_sum(double v, double *sh) {
    v = sum64(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}
__device__ __forceinline__ double block_max(double v, double *sh) {
    v = max64(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmax(fmax(sh[0], sh[1]), fmax(sh[2], sh[3]));
}
}  // namespace

// HBM class: pruning, renormalisation, chaos, power and renormalisation of one column of the expanded matrix per workgroup, in
// place; chaos_col[col0 + j] = the column's chaos.  A thread touches its own rows only
__global__ void __launch_bounds__(MCL_THREADS) k_mcl_inflate(const MclComp *comps, const int *active, double *pool, int parity, MclRun run, double *chaos_col) {
    const MclComp c = comps[active[blockIdx.y]];
    const int j = (int)blockIdx.x, n = c.n;
    if (j >= n) return;
    __shared__ double sh[4];
    const size_t ld = (size_t)c.npad;
    double *col = pool + c.mat + (parity ? 0 : ld * ld) + (size_t)j * ld;
    const double thr = 1.0 / run.prune_inverse;
    double s = 0;
    for (int i = (int)threadIdx.x; i < n; i += MCL_THREADS) { double x = col[i]; if (x < thr) x = 0.0; col[i] = x; s += x; }
    s = block_sum(s, sh);
    double mx = 0, sq = 0;
    for (int i = (int)threadIdx.x; i < n; i += MCL_THREADS) { const double x = s > 0 ? col[i] / s : 0.0; col[i] = x; mx = fmax(mx, x); sq += x * x; }
    mx = block_max(mx, sh); sq = block_sum(sq, sh);
    double s2 = 0;
    for (int i = (int)threadIdx.x; i < n; i += MCL_THREADS) { const double x = col[i]; const double p = x > 0 ? pow(x, run.inflation) : 0.0; col[i] = p; s2 += p; }
    s2 = block_sum(s2, sh);
    for (int i = (int)threadIdx.x; i < n; i += MCL_THREADS) col[i] = s2 > 0 ? col[i] / s2 : 0.0;
    if (threadIdx.x == 0) chaos_col[c.col0 + j] = mx - sq;
}

// one workgroup per active component: its chaos (a maximum: exact in any order), the iterations it has made, its flag
__global__ void __launch_bounds__(MCL_THREADS) k_mcl_flag(const MclComp *comps, const int *active, const double *chaos_col, MclRun run, int it, int *iters,
                                                          double *chaos_out, int *flag) {
    const int ci = active[blockIdx.x];
    const MclComp c = comps[ci];
    __shared__ double sh[4];
    double mx = -1e300;
    for (int j = (int)threadIdx.x; j < c.n; j += MCL_THREADS) mx = fmax(mx, chaos_col[c.col0 + j]);
    mx = block_max(mx, sh);
    if (threadIdx.x == 0) { iters[ci] = it; chaos_out[ci] = mx; flag[blockIdx.x] = mx < run.chaos_eps ? 1 : 0; }
}

// HBM class: the reading of a component's final matrix (buffer B after an odd number of iterations), one workgroup per column
__global__ void __launch_bounds__(MCL_THREADS) k_mcl_read(const MclComp *comps, const double *pool, const int *iters, int *best, unsigned *mask) {
    const MclComp c = comps[blockIdx.y];
    const int j = (int)blockIdx.x, n = c.n;
    if (j >= n) return;
    const size_t ld = (size_t)c.npad;
    const double *M = pool + c.mat + ((iters[blockIdx.y] & 1) ? ld * ld : 0);
    const double *col = M + (size_t)j * ld;
    __shared__ double s_v[4];
    __shared__ int s_i[4];
    double bv = 0; int bi = -1;
    for (int i = (int)threadIdx.x; i < n; i += MCL_THREADS) if (M[(size_t)i * ld + i] > 0) better(bv, bi, col[i], i);
    for (int m = 32; m >= 1; m >>= 1) { const double v2 = shfl_xor_d(bv, m); const int i2 = __shfl_xor(bi, m); better(bv, bi, v2, i2); }
    if ((threadIdx.x & 63) == 0) { s_v[threadIdx.x >> 6] = bv; s_i[threadIdx.x >> 6] = bi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < 4; ++k) better(bv, bi, s_v[k], s_i[k]);
        best[c.col0 + j] = bi;
    }
    const int W = (n + 31) >> 5;
    const bool att_j = col[j] > 0;
    for (int w = (int)threadIdx.x; w < W; w += MCL_THREADS) {
        unsigned bits = 0;
        if (att_j)
            for (int b = 0; b < 32; ++b) { const int i = 32 * w + b; if (i < n && M[(size_t)i * ld + i] > 0 && col[i] > 0) bits |= 1u << b; }
        mask[c.mask_off + (size_t)j * W + w] = bits;
    }
}

size_t mcl_lds_bytes(bool packed) {
    return packed ? (size_t)4 * 2 * MCL_PACKED_MAX * (MCL_PACKED_MAX + 2) * sizeof(double) : (size_t)2 * MCL_LDS_MAX * MCL_LDS_LD * sizeof(double);
}

void launch_mcl_fill(const MclComp *comps, int ncomps, int max_n, const long long *ptr, const int *row, const double *val, double *pool, hipStream_t s) {
    if (ncomps < 1 || max_n < 1) return;
    hipLaunchKernelGGL(k_mcl_fill, dim3((unsigned)((max_n + 63) / 64), (unsigned)ncomps), dim3(64), 0, s, comps, ptr, row, val, pool);
}

hipError_t launch_mcl_lds(bool packed, const MclComp *comps, int ncomps, double *pool, const MclRun &run, int *best, unsigned *mask, int *iters, double *chaos,
                          bool write_back, hipStream_t s) {
    if (ncomps < 1) return hipSuccess;
    const size_t bytes = mcl_lds_bytes(packed);
    if (packed) {
        hipLaunchKernelGGL(k_mcl_lds<true>, dim3((unsigned)((ncomps + 3) / 4)), dim3(MCL_THREADS), bytes, s, comps, ncomps, pool, run, best, mask, iters, chaos, write_back ? 1 : 0);
    } else {
        static const hipError_t big = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_mcl_lds<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)mcl_lds_bytes(false));
        if (big != hipSuccess) return big;
        hipLaunchKernelGGL(k_mcl_lds<false>, dim3((unsigned)ncomps), dim3(MCL_THREADS), bytes, s, comps, ncomps, pool, run, best, mask, iters, chaos, write_back ? 1 : 0);
    }
    return hipSuccess;
}

void launch_mcl_expand(const MclComp *comps, const int *active, int nactive, int max_npad, double *pool, int parity, hipStream_t s) {
    if (nactive < 1) return;
    const unsigned T = (unsigned)(max_npad / MCL_TILE);
    hipLaunchKernelGGL(k_mcl_expand, dim3(T, T, (unsigned)nactive), dim3(MCL_THREADS), 0, s, comps, active, pool, parity);
}

void launch_mcl_inflate(const MclComp *comps, const int *active, int nactive, int max_n, double *pool, int parity, const MclRun &run, double *chaos_col, hipStream_t s) {
    if (nactive < 1) return;
    hipLaunchKernelGGL(k_mcl_inflate, dim3((unsigned)max_n, (unsigned)nactive), dim3(MCL_THREADS), 0, s, comps, active, pool, parity, run, chaos_col);
}

void launch_mcl_flag(const MclComp *comps, const int *active, int nactive, const double *chaos_col, const MclRun &run, int it, int *iters, double *chaos, int *flag,
                     hipStream_t s) {
    if (nactive < 1) return;
    hipLaunchKernelGGL(k_mcl_flag, dim3((unsigned)nactive), dim3(MCL_THREADS), 0, s, comps, active, chaos_col, run, it, iters, chaos, flag);
}

void launch_mcl_read(const MclComp *comps, int ncomps, int max_n, const double *pool, const int *iters, int *best, unsigned *mask, hipStream_t s) {
    if (ncomps < 1) return;
    hipLaunchKernelGGL(k_mcl_read, dim3((unsigned)max_n, (unsigned)ncomps), dim3(MCL_THREADS), 0, s, comps, pool, iters, best, mask);
}

}  // namespace pml
