// msa.hip -- the multiple alignment's kernels (include/peprml.h "Multiple alignment"): one merge of two clusters is a task, and all
// tasks of one level of all sets of a call go through each kernel in one launch.
//
// k_msa_counts   the count profile of a call's starting clusters: 24 int16 a column (12 dwords), one thread per dword
// k_msa_colv     V_j[a] = Sum_b cY[j][b] T[a][b] of every column j of every task's Y, int16, laid out like the counts, so that a
//                cell's score is 12 v_dot2 (__builtin_amdgcn_sdot2) of a column of X's counts with V_j
// k_msa_dp       the model is k_sw_score.  A workgroup is one wavefront; a group of L = 16 / 32 / 64 consecutive lanes works on one
//                task (64 / L tasks of one class per workgroup, MsaBlock).  Lane l keeps the strip of T = MSA_STRIP columns of X
//                [(pass * L + l) * T, + T) in registers: their counts (96 dwords), H and E of the previous column of Y.  At step s
//                lane l works on column s - l of Y: an anti-diagonal pipeline; H and F of a strip's last row move down the lanes
//                with one DPP move each (wave_shr:1).  Every lane reads the V of its own column from HBM / L2 (48 B, three
//                dwordx4, one column ahead): adjacent lanes read adjacent columns, no LDS is used.  The four direction bits of
//                the strip's eight cells are one dword, stored at ((pass * nsteps + s) * L + l): a step's stores are coalesced
//     passes     LX > L * T (widest class only: a group is the wavefront): the last lane writes (H, F) of its last row per column
//                into one of two line buffers, lane 0 of the next pass reads the other one; a fence between the passes
//     boundary   H[i][0] = -i GE, E[i][0] = minus infinity; row 0 (lane 0, first pass) H[0][j] = -j GE, F[0][j] = minus infinity
//     rows       past LX have all-zero counts; nothing above them reads them
// k_msa_walk     the traceback: one lane per task follows the direction words from (LX, LY) and writes the merged column map from
//                its end; info[task].x = the merged length
// k_msa_gather   the merged cluster's rows and counts through the map, one thread per merged column
#include "kernels.h"
#include "msa.hpp"

namespace pml {

static_assert(MSA_STRIP == 8, "eight cells of four bits are one direction word");
static_assert(MSA_CW == 24, "12 dwords a column");

__device__ __forceinline__ int msa_lane_up(int v) { return __builtin_amdgcn_update_dpp(v, v, 0x138, 0xF, 0xF, false); }

typedef short msa_short2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ int msa_dot2(uint32_t a, uint32_t b, int c) {
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(msa_short2, a), __builtin_bit_cast(msa_short2, b), c, false);
}

__global__ __launch_bounds__(256) void k_msa_counts(const MsaCluster *__restrict__ clusters) {
    const MsaCluster c = clusters[blockIdx.x];
    for (long long t = (long long)blockIdx.y * 256 + threadIdx.x; t < (long long)c.L * 12; t += (long long)gridDim.y * 256) {
        const int col = (int)(t / 12), m = (int)(t % 12);
        uint32_t lo = 0, hi = 0;
        for (int r = 0; r < c.n; ++r) {
            const int a = c.rows[(size_t)r * c.L + col];
            lo += a == 2 * m; hi += a == 2 * m + 1 && a < MSA_GAP;
        }
        c.cnt[t] = lo | (hi << 16);
    }
}

__global__ __launch_bounds__(256) void k_msa_colv(const MsaTask *__restrict__ tasks, const int8_t *__restrict__ table576) {
    __shared__ int tab[576];
    for (int k = threadIdx.x; k < 576; k += 256) tab[k] = table576[k];
    __syncthreads();
    const MsaTask t = tasks[blockIdx.x];
    const int16_t *cy = (const int16_t *)t.y_cnt;
    int16_t *v = (int16_t *)t.v;
    for (long long e = (long long)blockIdx.y * 256 + threadIdx.x; e < (long long)t.LY * MSA_CW; e += (long long)gridDim.y * 256) {
        const int j = (int)(e / MSA_CW), a = (int)(e % MSA_CW);
        int acc = 0;
        if (a < MSA_GAP)
            for (int b = 0; b < MSA_GAP; ++b) acc += (int)cy[(size_t)j * MSA_CW + b] * tab[a * 24 + b];
        v[e] = (int16_t)acc;
    }
}

template <int L>
__device__ __forceinline__ void msa_dp_body(const MsaTask *__restrict__ tasks, const MsaBlock blk, int2 *info) {
    constexpr int T = MSA_STRIP, GPW = MSA_THREADS / L, NEG = MSA_NEG;
    const int lane = threadIdx.x, g = lane / L, gl = lane & (L - 1);
    const bool have = g < blk.count;
    MsaTask t = tasks[blk.first + (have ? g : 0)];
    if (!have) { t.LX = 0; t.LY = 0; }
    const int LX = t.LX, LY = t.LY, GE = t.GE, GOE = t.GO + t.GE;
    int maxLY = 0;
#pragma unroll
    for (int k = 0; k < GPW; ++k) maxLY = max(maxLY, __builtin_amdgcn_readlane(LY, k * L));
    const int npass = L == 64 ? max(1, __builtin_amdgcn_readfirstlane((LX + L * T - 1) / (L * T))) : 1;
    const int nsteps = maxLY + L - 1, tsteps = LY + L - 1;               // the wavefront's loop; the task's own steps (its direction words' stride)
    const uint4 *vcol = (const uint4 *)t.v;
    const int last_strip = (LX - 1) / T;
    for (int pass = 0; pass < npass; ++pass) {
        const bool first = pass == 0, last = pass == npass - 1;
        const int row0 = (pass * L + gl) * T;                            // the row above the strip (rows are 1-based)
        uint32_t cx[T][12];
        int H[T], E[T], oe[T];
#pragma unroll
        for (int k = 0; k < T; ++k) {
            const int i = row0 + k + 1;
            if (i <= LX) {
                const uint4 *p = (const uint4 *)(t.x_cnt + (size_t)(i - 1) * 12);
                const uint4 a = p[0], b = p[1], c = p[2];
                cx[k][0] = a.x; cx[k][1] = a.y; cx[k][2] = a.z; cx[k][3] = a.w; cx[k][4] = b.x; cx[k][5] = b.y; cx[k][6] = b.z; cx[k][7] = b.w;
                cx[k][8] = c.x; cx[k][9] = c.y; cx[k][10] = c.z; cx[k][11] = c.w;
            } else {
#pragma unroll
                for (int m = 0; m < 12; ++m) cx[k][m] = 0;
            }
            H[k] = -i * GE; E[k] = NEG;
            oe[k] = i == LX ? GE : GOE;
        }
        int diag = -row0 * GE;                                           // H[row0][0]
        int o_h = 0, o_f = 0;                                            // what the lane below reads at the next step
        int2 *lb_w = t.lb ? t.lb + (size_t)(pass & 1) * LY : nullptr;
        const int2 *lb_r = t.lb ? t.lb + (size_t)((pass + 1) & 1) * LY : nullptr;
        uint4 vn0 = make_uint4(0, 0, 0, 0), vn1 = vn0, vn2 = vn0;
        int2 ln = make_int2(0, 0);
        if (have && gl == 0 && LY > 0) {
            vn0 = vcol[0]; vn1 = vcol[1]; vn2 = vcol[2];
            if (!first) ln = lb_r[0];
        }
        for (int s = 0; s < nsteps; ++s) {
            const int jj = s - gl;                                       // this lane's column of Y, 0-based
            const bool valid = have && jj >= 0 && jj < LY;
            const uint4 v0 = vn0, v1 = vn1, v2 = vn2;
            const int2 lc = ln;
            const int jn = jj + 1;
            if (have && jn >= 0 && jn < LY) {
                vn0 = vcol[(size_t)jn * 3]; vn1 = vcol[(size_t)jn * 3 + 1]; vn2 = vcol[(size_t)jn * 3 + 2];
                if (!first && gl == 0) ln = lb_r[jn];
            }
            int hu = msa_lane_up(o_h), fu = msa_lane_up(o_f);
            if (gl == 0) { hu = first ? -(jj + 1) * GE : lc.x; fu = first ? NEG : lc.y; }
            if (valid) {
                const uint32_t vv[12] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w, v2.x, v2.y, v2.z, v2.w};
                const int of = jj + 1 == LY ? GE : GOE;
                int d = diag, h = hu, f = fu;
                uint32_t bits = 0;
                diag = hu;
#pragma unroll
                for (int k = 0; k < T; ++k) {
                    int sc = 0;
#pragma unroll
                    for (int m = 0; m < 12; ++m) sc = msa_dot2(cx[k][m], vv[m], sc);
                    const int fo = h - of, fx = f - GE;
                    f = max(fx, fo);
                    const int eo = H[k] - oe[k], ex = E[k] - GE;
                    const int e = max(ex, eo);
                    const int dg = d + sc, ef = max(e, f);
                    h = max(dg, ef);
                    const uint32_t src = dg >= ef ? 0u : (e >= f ? 1u : 2u);
                    bits |= (src | (eo >= ex ? 4u : 0u) | (fo >= fx ? 8u : 0u)) << (4 * k);
                    d = H[k]; H[k] = h; E[k] = e;
                }
                o_h = h; o_f = f;
                t.dir[((size_t)pass * tsteps + s) * L + gl] = bits;
                if (gl == L - 1 && !last) lb_w[jj] = make_int2(h, f);
            }
        }
        if (last && have && gl == (last_strip & (L - 1)) && (last_strip / L) == pass) {
            int sc = H[0];
#pragma unroll
            for (int k = 1; k < T; ++k) sc = ((LX - 1) & (T - 1)) == k ? H[k] : sc;
            info[blk.first + g].y = sc;
        }
        if (!last) __threadfence();                                      // the line buffer's writes before the next pass's reads
    }
}

__global__ __launch_bounds__(MSA_THREADS) void k_msa_dp(const MsaTask *__restrict__ tasks, const MsaBlock *__restrict__ blocks, int2 *info) {
    const MsaBlock blk = blocks[blockIdx.x];
    if (blk.cls == 0) msa_dp_body<16>(tasks, blk, info);
    else if (blk.cls == 1) msa_dp_body<32>(tasks, blk, info);
    else msa_dp_body<64>(tasks, blk, info);
}

__global__ __launch_bounds__(64) void k_msa_walk(const MsaTask *__restrict__ tasks, int ntasks, int2 *info) {
    const int ti = blockIdx.x * 64 + threadIdx.x;
    if (ti >= ntasks) return;
    const MsaTask t = tasks[ti];
    const int L = t.cls == 0 ? 16 : t.cls == 1 ? 32 : 64;
    const size_t tsteps = (size_t)t.LY + L - 1;
    int i = t.LX, j = t.LY, state = 0;
    int pos = t.LX + t.LY;
    size_t at = (size_t)-1;
    uint32_t w = 0;
    while (i > 0 && j > 0) {
        const int strip = (i - 1) >> 3, p = strip / L, l = strip & (L - 1);
        const size_t idx = ((size_t)p * tsteps + (size_t)(j - 1 + l)) * L + l;
        if (idx != at) { w = t.dir[idx]; at = idx; }
        const uint32_t nib = (w >> (4 * ((i - 1) & 7))) & 15u;
        if (state == 0) state = (int)(nib & 3u);
        if (state == 0) { t.map[--pos] = make_int2(i - 1, j - 1); --i; --j; }
        else if (state == 1) { t.map[--pos] = make_int2(-1, j - 1); if (nib & 4u) state = 0; --j; }
        else { t.map[--pos] = make_int2(i - 1, -1); if (nib & 8u) state = 0; --i; }
    }
    for (; j > 0; --j) t.map[--pos] = make_int2(-1, j - 1);
    for (; i > 0; --i) t.map[--pos] = make_int2(i - 1, -1);
    info[ti].x = t.LX + t.LY - pos;
}

__global__ __launch_bounds__(256) void k_msa_gather(const MsaTask *__restrict__ tasks, const int2 *__restrict__ info) {
    const MsaTask t = tasks[blockIdx.x];
    const int Lm = info[blockIdx.x].x;
    const int2 *map = t.map + (t.LX + t.LY - Lm);
    for (int c = blockIdx.y * 256 + threadIdx.x; c < Lm; c += gridDim.y * 256) {
        const int2 ij = map[c];
        for (int r = 0; r < t.nX; ++r) t.out_rows[(size_t)r * Lm + c] = ij.x >= 0 ? t.x_rows[(size_t)r * t.LX + ij.x] : (uint8_t)MSA_GAP;
        for (int r = 0; r < t.nY; ++r) t.out_rows[(size_t)(t.nX + r) * Lm + c] = ij.y >= 0 ? t.y_rows[(size_t)r * t.LY + ij.y] : (uint8_t)MSA_GAP;
        for (int m = 0; m < 12; ++m)                                     // two int16 counts a dword: their sums stay below 2^16, no carry
            t.out_cnt[(size_t)c * 12 + m] = (ij.x >= 0 ? t.x_cnt[(size_t)ij.x * 12 + m] : 0u) + (ij.y >= 0 ? t.y_cnt[(size_t)ij.y * 12 + m] : 0u);
    }
}

static unsigned tiles_of(long long items) { return (unsigned)std::min<long long>(std::max<long long>((items + 255) / 256, 1), 65535); }

void launch_msa_counts(const MsaCluster *clusters, int nclusters, int max_L, hipStream_t s) {
    if (nclusters <= 0) return;
    hipLaunchKernelGGL(k_msa_counts, dim3((unsigned)nclusters, tiles_of((long long)max_L * 12)), dim3(256), 0, s, clusters);
}
void launch_msa_colv(const MsaTask *tasks, int ntasks, int max_LY, const int8_t *table576, hipStream_t s) {
    if (ntasks <= 0) return;
    hipLaunchKernelGGL(k_msa_colv, dim3((unsigned)ntasks, tiles_of((long long)max_LY * MSA_CW)), dim3(256), 0, s, tasks, table576);
}
void launch_msa_dp(const MsaTask *tasks, const MsaBlock *blocks, int nblocks, int2 *info, hipStream_t s) {
    if (nblocks <= 0) return;
    hipLaunchKernelGGL(k_msa_dp, dim3((unsigned)nblocks), dim3(MSA_THREADS), 0, s, tasks, blocks, info);
}
void launch_msa_walk(const MsaTask *tasks, int ntasks, int2 *info, hipStream_t s) {
    if (ntasks <= 0) return;
    hipLaunchKernelGGL(k_msa_walk, dim3((unsigned)((ntasks + 63) / 64)), dim3(64), 0, s, tasks, ntasks, info);
}
void launch_msa_gather(const MsaTask *tasks, int ntasks, int max_L, const int2 *info, hipStream_t s) {
    if (ntasks <= 0) return;
    hipLaunchKernelGGL(k_msa_gather, dim3((unsigned)ntasks, tiles_of(max_L)), dim3(256), 0, s, tasks, info);
}

}  // namespace pml
