// rell.hip -- multiscale RELL resampling for the tree selection tests (AU / KH / SH / BP; kernels.h RellReq).
//
// k_rell: one thread owns one replicate (scale k, replicate b): it hashes its n_k draws, gathers the drawn rows of the
// per-site lnL table and adds them, in draw order, into T sums that live in its registers -- so a sum's bits depend on
// (seed, k, b, N, X) alone.  The kernel is instantiated per row width (tpad = 2 .. 64) so that the sums are a register
// array and a row is read with unguarded 16-byte loads.  Work per draw: one mix64 (two 64-bit multiplies, ~25 VALU
// instructions), tpad / 2 16-byte gathers, tpad f64 adds; no store.  The statistics are counted in the epilogue: ballots
// per wave, one LDS add per wave and counter, one global 64-bit integer atomic per workgroup and counter.
//
// Two paths, same bits:
//   LDS     every workgroup copies the table into dynamic LDS once (N * slots * 16 bytes, slots = tpad / 2 rounded up to odd)
//           and gathers with ds_read_b128.  The drawn rows are random, so no layout removes bank conflicts; what a layout
//           can do is not to add any: ds_read_b128 serves a 16-lane group from the 16 16-byte slots of a 256-byte bank row,
//           and slot i of row s sits at (slots * s + i) mod 16 -- with an even row width the 16 lanes of a group would share
//           16 / gcd(slots, 16) slots (tpad = 16: two of them, 8-way); an odd width spreads them over all 16 (the expected
//           worst slot of 16 random lanes holds ~3).
//   global  the same gathers from HBM addresses: the table of a concatenation (100 000 sites x 10 trees = 8 MB) stays in
//           L2 / Infinity Cache.
//
// The weighted arm (k_rell<TC, LDS, true>, RellWReq) is a further instantiation of the same body for the calls that ask for
// wKH / wSH: everything above happens exactly as in the plain arm, then the epilogue of scale k1 turns the sums into C_t in
// place and counts, for every t, max_u (C_u - C_t) / sigma_ut against its observed value -- T^2 multiply-compares per
// replicate; the loop over u is fully unrolled, so the sums stay registers.  1 / sigma_ut (k_rell_pairsd) sits in dynamic LDS behind the
// table (or alone on the global path); row t is read with ds_read_b128 at one address for the whole wave, which the LDS
// broadcasts.  What depends on t alone (S_t, u*, the set of usable u) is worked out once per workgroup by its first wave.
#include "kernels.h"

#include <algorithm>

namespace pml {

constexpr int RELL_BS = 512;            // 8 waves: two per SIMD and up to 256 VGPRs each (tpad = 64: 128 of them are sums)
constexpr int RELL_STATIC_LDS = 2048;   // s_L + s_cnt below, rounded up
constexpr int RELL_W_STATIC_LDS = 4096; // the weighted arm: two more counters, s_S, s_us, s_m
constexpr size_t rell_isig_bytes(int tpad) { return (size_t)tpad * tpad * sizeof(double); }

// C_t = Y_t * (N / n_k) - L_t as two rounded operations (the reference of the tests does the same two)
__device__ __forceinline__ double rell_centre(double y, double scale, double l) {
#pragma clang fp contract(off)
    const double ys = y * scale;
    return ys - l;
}

// a 64-bit value that every lane of the wave holds alike, moved to scalar registers: what tests it is then a scalar branch
__device__ __forceinline__ unsigned long long rell_uniform(unsigned long long v) {
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return ((unsigned long long)hi << 32) | lo;
}
// (a - b) / sigma as two rounded operations: the difference, then its product with 1 / sigma
__device__ __forceinline__ double rell_ratio(double a, double b, double inv_sigma) {
#pragma clang fp contract(off)
    const double d = a - b;
    return d * inv_sigma;
}

template <bool W> struct RellArg { using type = RellReq; };
template <> struct RellArg<true> { using type = RellWReq; };

template <int TC, bool LDS, bool W = false>
__global__ __launch_bounds__(RELL_BS) void k_rell(const typename RellArg<W>::type r) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    __shared__ double s_L[64];
    __shared__ unsigned s_cnt[W ? 5 : 3][64];   // bp, kh, sh (weighted arm: wkh, wsh) of this workgroup
    __shared__ double s_S[W ? 64 : 1];               // weighted arm: S_t, the observed maximum
    __shared__ int s_us[W ? 64 : 1];                 //   u*(t), -1 if t has no pair
    __shared__ unsigned long long s_m[W ? 64 : 1];   //   bit u: the pair (u, t) is used
    constexpr int TP2 = TC / 2;
    const int tid = threadIdx.x, lane = tid & 63;
    const unsigned bpk = (unsigned)(((unsigned long long)r.B + RELL_BS - 1) / RELL_BS);          // workgroups per scale
    const int k = (int)(blockIdx.x / bpk);
    const unsigned b = (blockIdx.x % bpk) * RELL_BS + (unsigned)tid;
    const int T = r.T;
    double2 *s_tab = reinterpret_cast<double2 *>(s_raw);
    constexpr int RS = LDS ? rell_lds_slots(TC) : TP2;           // row stride in 16-byte slots
    if (LDS) {
        const double2 *X2 = reinterpret_cast<const double2 *>(r.X);
        const int total = r.N * TP2;
        for (int e = tid; e < total; e += RELL_BS) { const int s = e / TP2, i = e - s * TP2; s_tab[s * RS + i] = X2[e]; }
    }
    double2 *s_is2 = nullptr;
    if constexpr (W) {
        s_is2 = reinterpret_cast<double2 *>(s_raw + (LDS ? rell_lds_bytes(r.N, TC) : 0));
        const double2 *g = reinterpret_cast<const double2 *>(r.isig);
        for (int e = tid; e < TC * TP2; e += RELL_BS) s_is2[e] = g[e];
    }
    if (tid < 64) s_L[tid] = tid < T ? r.L[tid] : 0.0;
    if (tid < (W ? 5 : 3) * 64) (&s_cnt[0][0])[tid] = 0u;
    __syncthreads();
    if constexpr (W) {
        if (k == r.k1 && tid < T) {
            const double *is = reinterpret_cast<const double *>(s_is2) + tid * TC;
            const double Lt = s_L[tid];
            double S = -HUGE_VAL; int us = -1; unsigned long long m = 0ull;
            for (int u = 0; u < T; ++u) {
                const double w = is[u];
                if (u == tid || !(w > 0.0)) continue;
                const double q = rell_ratio(s_L[u], Lt, w);
                m |= 1ull << u;
                if (q > S) { S = q; us = u; }
            }
            s_S[tid] = S; s_us[tid] = us; s_m[tid] = m;
        }
        __syncthreads();
    }

    const bool valid = b < r.B;
    double acc[TC];
#pragma unroll
    for (int t = 0; t < TC; ++t) acc[t] = 0.0;
    if (valid) {
        const int nk = r.ndraws[k];
        const unsigned long long key = r.base + (((unsigned long long)k * r.B + b) << 32);
        const unsigned N = (unsigned)r.N;
        const double2 *tab = LDS ? s_tab : reinterpret_cast<const double2 *>(r.X);
#pragma unroll 2
        for (int j = 0; j < nk; ++j) {
            const unsigned long long h = mix64(key + (unsigned long long)j);
            const unsigned site = __umulhi((unsigned)(h >> 32), N);
            const double2 *row = tab + (size_t)site * RS;
#pragma unroll
            for (int i = 0; i < TP2; ++i) { const double2 v = row[i]; acc[2 * i] += v.x; acc[2 * i + 1] += v.y; }
        }
        if (r.Y) {
            double *y = r.Y + ((size_t)k * r.B + b) * (size_t)T;
#pragma unroll
            for (int t = 0; t < TC; ++t) if (t < T) y[t] = acc[t];
        }
    }

    // bootstrap probability: the replicate votes for its best tree (lowest index of equals)
    int arg = 0; double best = acc[0];
#pragma unroll
    for (int t = 1; t < TC; ++t) if (t < T && acc[t] > best) { best = acc[t]; arg = t; }
    for (int t = 0; t < T; ++t) {
        const unsigned long long m = __ballot(valid && arg == t);
        if (lane == 0 && m) atomicAdd(&s_cnt[0][t], (unsigned)__popcll(m));
    }
    if (k == r.k1) {
        // a = the best tree, a2 = the best of the others (lowest index of equals): u*(t) = a for every t but a, a2 for a
        int a = 0;
        for (int t = 1; t < T; ++t) if (s_L[t] > s_L[a]) a = t;
        int a2 = a == 0 ? 1 : 0;
        for (int t = a2 + 1; t < T; ++t) if (t != a && s_L[t] > s_L[a2]) a2 = t;
        const double scale = r.scale[k], La = s_L[a], La2 = s_L[a2];
        double maxC = 0.0, Ca = 0.0, Ca2 = 0.0;
#pragma unroll
        for (int t = 0; t < TC; ++t) if (t < T) {
            const double c = rell_centre(acc[t], scale, s_L[t]);
            maxC = t == 0 ? c : fmax(maxC, c);
            if (t == a) Ca = c;
            if (t == a2) Ca2 = c;
        }
#pragma unroll
        for (int t = 0; t < TC; ++t) if (t < T) {
            const double c = rell_centre(acc[t], scale, s_L[t]), Lt = s_L[t];
            const bool sh = maxC - c >= La - Lt;
            const bool kh = (t == a ? Ca2 : Ca) - c >= (t == a ? La2 : La) - Lt;
            const unsigned long long mk = __ballot(valid && kh), ms = __ballot(valid && sh);
            if (lane == 0 && mk) atomicAdd(&s_cnt[1][t], (unsigned)__popcll(mk));
            if (lane == 0 && ms) atomicAdd(&s_cnt[2][t], (unsigned)__popcll(ms));
        }
        if constexpr (W) {
#pragma unroll
            for (int t = 0; t < TC; ++t) acc[t] = rell_centre(acc[t], scale, s_L[t]);      // the sums are done with: C_t in their place
            // t is a loop at run time (T^2 unrolled bodies would be 4096 at T = 64): C_t comes out of the register array by a chain
            // of selects on the wave-uniform t, and the loop over u stays unrolled
#pragma unroll 1
            for (int t = 0; t < T; ++t) {
                const unsigned long long m = rell_uniform(s_m[t]);            // u = t and the padding are not in it
                const int us = __builtin_amdgcn_readfirstlane(s_us[t]);
                const double St = s_S[t];
                const double2 *row = s_is2 + t * TP2;                // row t = column t: the matrix is symmetric
                double ct = acc[0];
#pragma unroll
                for (int u = 1; u < TC; ++u) ct = u == t ? acc[u] : ct;
                double best = -HUGE_VAL, qk = 0.0;
#pragma unroll
                for (int i = 0; i < TP2; ++i) {
                    const double2 w = row[i];
                    if ((m >> (2 * i)) & 1ull) {
                        const double q = rell_ratio(acc[2 * i], ct, w.x);
                        best = fmax(best, q);
                        if (us == 2 * i) qk = q;
                    }
                    if ((m >> (2 * i + 1)) & 1ull) {
                        const double q = rell_ratio(acc[2 * i + 1], ct, w.y);
                        best = fmax(best, q);
                        if (us == 2 * i + 1) qk = q;
                    }
                }
                const bool wsh = m == 0ull || best >= St, wkh = m == 0ull || qk >= St;      // S_t is also the observed ratio of u*
                const unsigned long long mk = __ballot(valid && wkh), ms = __ballot(valid && wsh);
                if (lane == 0 && mk) atomicAdd(&s_cnt[3][t], (unsigned)__popcll(mk));
                if (lane == 0 && ms) atomicAdd(&s_cnt[4][t], (unsigned)__popcll(ms));
            }
        }
    }
    __syncthreads();
    if (tid < T) {
        if (s_cnt[0][tid]) atomicAdd(&r.bp[(size_t)k * T + tid], (unsigned long long)s_cnt[0][tid]);
        if (k == r.k1) {
            if (s_cnt[1][tid]) atomicAdd(&r.kh[tid], (unsigned long long)s_cnt[1][tid]);
            if (s_cnt[2][tid]) atomicAdd(&r.sh[tid], (unsigned long long)s_cnt[2][tid]);
            if constexpr (W) {
                if (s_cnt[3][tid]) atomicAdd(&r.wkh[tid], (unsigned long long)s_cnt[3][tid]);
                if (s_cnt[4][tid]) atomicAdd(&r.wsh[tid], (unsigned long long)s_cnt[4][tid]);
            }
        }
    }
}

// the table: one thread per site
__global__ __launch_bounds__(256) void k_rell_pack(const double *const *__restrict__ src, const int *__restrict__ site2pat,
                                                   double *__restrict__ X, int N, int T, int tpad) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= N) return;
    const int p = site2pat ? site2pat[s] : s;
    double *row = X + (size_t)s * tpad;
    for (int t = 0; t < T; ++t) row[t] = src[t][p];
    for (int t = T; t < tpad; ++t) row[t] = 0.0;
}
// L[t] = sum_s X[s][t], s ascending: one thread per tree (a row of the table is one coalesced read of the wave)
__global__ __launch_bounds__(64) void k_rell_colsum(const double *__restrict__ X, double *__restrict__ L, int N, int T, int tpad) {
    const int t = threadIdx.x;
    if (t >= T) return;
    double sum = 0.0;
    const double *p = X + t;
    int s = 0;
    for (; s + 8 <= N; s += 8) {
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = p[(size_t)(s + u) * tpad];
#pragma unroll
        for (int u = 0; u < 8; ++u) sum += v[u];
    }
    for (; s < N; ++s) sum += p[(size_t)s * tpad];
    L[t] = sum;
}

// 1 / sigma_ut (kernels.h launch_rell_pairsd): workgroup = one 4 x 4 tile of pairs (u in tile bi, t in tile bj, bi <= bj); a thread
// reads the two 32-byte pieces of a row once for the tile's 16 differences; pass 0 sums d, pass 1 sums (d - mean)^2.  A sum
// is reduced in a fixed order: lanes by shuffles, waves through LDS.
constexpr int PSD_BS = 512;
__global__ __launch_bounds__(PSD_BS) void k_rell_pairsd(const double *__restrict__ X, double *__restrict__ isig, int N, int T, int tpad) {
    __shared__ double s_part[PSD_BS / 64][16];
    __shared__ double s_mean[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int bj = 0, bi = (int)blockIdx.x;
    while (bi > bj) { bi -= bj + 1; ++bj; }                     // tiles row by row of the triangle: at most 16 rows
    const int u0 = 4 * bi, t0 = 4 * bj, tp2 = tpad / 2;
    const bool u2 = u0 + 2 < tpad, t2 = t0 + 2 < tpad;          // the tile's second 16-byte piece lies inside the row
    const double2 *X2 = reinterpret_cast<const double2 *>(X);
    double mean[16], sum[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) mean[q] = 0.0;
    for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
        for (int q = 0; q < 16; ++q) sum[q] = 0.0;
#pragma unroll 2
        for (int s = tid; s < N; s += PSD_BS) {
            const double2 *row = X2 + (size_t)s * tp2;
            const double2 zero = make_double2(0.0, 0.0);
            const double2 a0 = row[u0 / 2], a1 = u2 ? row[u0 / 2 + 1] : zero, b0 = row[t0 / 2], b1 = t2 ? row[t0 / 2 + 1] : zero;
            const double xu[4] = {a0.x, a0.y, a1.x, a1.y}, xt[4] = {b0.x, b0.y, b1.x, b1.y};
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const double e = (xu[i] - xt[j]) - mean[4 * i + j];          // pass 0: mean = 0
                    sum[4 * i + j] += pass ? e * e : e;
                }
        }
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            double v = sum[q];
            for (int off = 32; off; off >>= 1) v += __shfl_down(v, off);
            if (lane == 0) s_part[wave][q] = v;
        }
        __syncthreads();
        double tot = 0.0;
        if (tid < 16) for (int w = 0; w < PSD_BS / 64; ++w) tot += s_part[w][tid];
        if (pass == 0) {
            if (tid < 16) s_mean[tid] = tot / (double)N;
            __syncthreads();
#pragma unroll
            for (int q = 0; q < 16; ++q) mean[q] = s_mean[q];
        } else if (tid < 16) {
            const int u = u0 + tid / 4, t = t0 + tid % 4;
            if (u < tpad && t < tpad && u <= t) {               // u > t happens in a diagonal tile only: the mirror of another thread's pair
                double v = 0.0;
                if (u != t && t < T && N > 1 && tot > 0.0) v = 1.0 / sqrt(tot * ((double)N / (double)(N - 1)));
                isig[(size_t)u * tpad + t] = v;
                isig[(size_t)t * tpad + u] = v;
            }
        }
    }
}

void launch_rell_pairsd(const double *X, double *isig, int N, int T, int tpad, hipStream_t s) {
    const int nt = (tpad + 3) / 4;
    hipLaunchKernelGGL(k_rell_pairsd, dim3((unsigned)(nt * (nt + 1) / 2)), dim3(PSD_BS), 0, s, X, isig, N, T, tpad);
}

void launch_rell_pack(const double *const *src, const int *site2pat, double *X, double *L, int N, int T, int tpad, hipStream_t s) {
    hipLaunchKernelGGL(k_rell_pack, dim3((unsigned)(((long long)N + 255) / 256)), dim3(256), 0, s, src, site2pat, X, N, T, tpad);
    hipLaunchKernelGGL(k_rell_colsum, dim3(1), dim3(64), 0, s, X, L, N, T, tpad);
}

bool rell_lds_fits(int N, int tpad, int device) {
    int cap = 0;
    if (hipDeviceGetAttribute(&cap, hipDeviceAttributeMaxSharedMemoryPerBlock, device) != hipSuccess) return false;
    const size_t room = (size_t)std::min(cap, 160 * 1024) - RELL_STATIC_LDS;
    return rell_lds_bytes(N, tpad) <= room;
}

bool rell_weighted_lds_fits(int N, int tpad, int device) {
    int cap = 0;
    if (hipDeviceGetAttribute(&cap, hipDeviceAttributeMaxSharedMemoryPerBlock, device) != hipSuccess) return false;
    const size_t room = (size_t)std::min(cap, 160 * 1024) - RELL_W_STATIC_LDS;
    return rell_lds_bytes(N, tpad) + rell_isig_bytes(tpad) <= room;
}

template <int TC, bool W, class Req>
static hipError_t launch_rell_t(const Req &r, bool lds, unsigned grid, hipStream_t s) {
    if (lds) {
        const size_t bytes = rell_lds_bytes(r.N, TC) + (W ? rell_isig_bytes(TC) : 0);
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_rell<TC, true, W>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (e != hipSuccess) { (void)hipGetLastError(); return e; }       // the refusal is reported here; it must not stick to the thread for the caller's retry
        hipLaunchKernelGGL((k_rell<TC, true, W>), dim3(grid), dim3(RELL_BS), bytes, s, r);
    } else {
        hipLaunchKernelGGL((k_rell<TC, false, W>), dim3(grid), dim3(RELL_BS), W ? rell_isig_bytes(TC) : 0, s, r);
    }
    return hipGetLastError();
}

template <bool W, class Req>
static hipError_t launch_rell_any(const Req &r, bool lds, hipStream_t s) {
    if (r.T < 2 || r.T > 64 || r.tpad != ((r.T + 1) & ~1) || r.N <= 0 || r.K <= 0 || r.B == 0) return hipErrorInvalidValue;
    const unsigned long long blocks = (unsigned long long)r.K * (((unsigned long long)r.B + RELL_BS - 1) / RELL_BS);
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    const unsigned grid = (unsigned)blocks;
    switch (r.tpad) {
#define RELL_CASE(TC) case TC: return launch_rell_t<TC, W>(r, lds, grid, s);
        RELL_CASE(2) RELL_CASE(4) RELL_CASE(6) RELL_CASE(8) RELL_CASE(10) RELL_CASE(12) RELL_CASE(14) RELL_CASE(16)
        RELL_CASE(18) RELL_CASE(20) RELL_CASE(22) RELL_CASE(24) RELL_CASE(26) RELL_CASE(28) RELL_CASE(30) RELL_CASE(32)
        RELL_CASE(34) RELL_CASE(36) RELL_CASE(38) RELL_CASE(40) RELL_CASE(42) RELL_CASE(44) RELL_CASE(46) RELL_CASE(48)
        RELL_CASE(50) RELL_CASE(52) RELL_CASE(54) RELL_CASE(56) RELL_CASE(58) RELL_CASE(60) RELL_CASE(62) RELL_CASE(64)
#undef RELL_CASE
    }
    return hipErrorInvalidValue;
}

hipError_t launch_rell(const RellReq &r, bool lds, hipStream_t s) { return launch_rell_any<false>(r, lds, s); }
hipError_t launch_rell_weighted(const RellWReq &r, bool lds, hipStream_t s) {
    if (!r.isig || !r.wkh || !r.wsh) return hipErrorInvalidValue;
    return launch_rell_any<true>(r, lds, s);
}

}  // namespace pml
