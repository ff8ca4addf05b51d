// sw.hip -- the homology search's score kernel (include/peprml.h "Homology search"): affine-gap Smith-Waterman of one query against
// a chunk of one genome's subjects, exact int32, with the per-genome selection folded in.
//
// k_sw_score<L>
//   grid    (blocks of 256 / L queries of the class, chunk); every group of a workgroup works on the SAME chunk
//   group   L = 16 / 32 / 64 consecutive lanes, one (query, chunk) task.  Lane l keeps the strip of T = SW_STRIP query rows
//           [pass * L * T + l * T, + T) in registers: H and E of the previous column and the rows' table offsets
//   stream  the chunk's subjects back to back, SW_MARK behind each.  At step s lane l works on stream position s - l: a systolic
//           anti-diagonal pipeline that fills and drains once per chunk.  The wavefront loads 64 stream bytes at a time, one
//           per lane and a batch ahead, and lane 0 of every group takes its byte from them by v_readlane (the step is
//           wavefront uniform); the byte then moves down the lanes beside H and F of the strip's last row, each with ONE DPP
//           move (wave_shr:1) -- no LDS round trip
//   marker  a step on SW_MARK subtracts SW_BIG everywhere, which leaves H = 0 and E, F <= 0 in every row (an E or F that is not
//           positive never wins against the 0 in H and never turns positive again without a positive H, so it stands for minus
//           infinity): the state is reset without a branch.  On that step the H channel carries the subject's running maximum
//           down the lanes instead: each lane passes on max(incoming, its own) and forgets its own
//   passes  a query longer than L * T rows (widest class only: a group is a wavefront) takes several passes over the chunk.  The
//           last lane writes H / F of its last row -- on a marker, the maximum so far -- per stream position into a line buffer
//           in HBM, which lane 0 of the next pass reads (coalesced batches of 64 positions, read before the pass overwrites
//           them in place; a fence between the passes)
//   rows    past the query's end use an all-zero table row: with costs >= 0 their cells never exceed the real cells above
//   LDS     the table as int8[25][32] (800 B): row 24 the padding row, column 24 the marker's
//   result  the last lane of the last pass receives every subject's score on the subject's marker, keeps the largest key
//           (S << 32 | 0xFFFFFFFF - position in the genome) and issues ONE 64-bit atomicMax into best[query][genome]: the result
//           does not depend on the order of the atomics
#include "kernels.h"

namespace pml {

static_assert(SW_TROWS * SW_TSTRIDE % 4 == 0 && SW_TROWS * SW_TSTRIDE / 4 <= SW_THREADS, "one thread copies one word of the table");
static_assert(SW_MARK < SW_TSTRIDE && SW_PAD_ROW < SW_TROWS, "the marker's column and the padding row lie inside the LDS table");
static_assert((long long)SW_MAX_LEN * 127 + 2LL * SW_BIG + (1 << 21) < (1LL << 31), "scores and the marker's subtraction fit int32");

// lane i takes lane i - 1's value (lane 0 keeps its own): v_mov_b32_dpp wave_shr:1
__device__ __forceinline__ int lane_up(int v) { return __builtin_amdgcn_update_dpp(v, v, 0x138, 0xF, 0xF, false); }

template <int L>
__global__ __launch_bounds__(SW_THREADS) void k_sw_score(const SwQuery *__restrict__ queries, const SwChunk *__restrict__ chunks, SwRun run,
                                                         const uint8_t *__restrict__ codes, const uint8_t *__restrict__ stream, const int *__restrict__ sub_pos,
                                                         const int8_t *__restrict__ table, int2 *linebuf, unsigned long long *best, int *dbg) {
    constexpr int T = SW_STRIP, GPB = SW_THREADS / L;
    __shared__ __attribute__((aligned(16))) int8_t tab[SW_TROWS * SW_TSTRIDE];
    const int tid = threadIdx.x;
    if (tid < SW_TROWS * SW_TSTRIDE / 4) ((uint32_t *)tab)[tid] = ((const uint32_t *)table)[tid];
    __syncthreads();
    const SwChunk ch = chunks[run.chunk0 + blockIdx.y];
    const int lane = tid & 63, gl = tid & (L - 1);
    const int qi = blockIdx.x * GPB + tid / L;
    const bool have = qi < run.nq;                                       // a group past the class's queries runs on an empty query
    SwQuery q; q.off = 0; q.len = 0; q.index = 0; q.lb_off = -1;
    if (have) q = queries[qi];
    const int npass = L == 64 ? (q.len > L * T ? (q.len + L * T - 1) / (L * T) : 1) : 1;      // wavefront uniform
    const uint8_t *sp = stream + ch.off;
    const int len = ch.len, nsteps = len + L - 1;
    int2 *lb = q.lb_off >= 0 ? linebuf + q.lb_off + ((long long)ch.lb_at - run.lb_base) : nullptr;
    unsigned long long kbest = 0;
    for (int pass = 0; pass < npass; ++pass) {
        const bool first = pass == 0, last = pass == npass - 1;
        int qidx[T], H[T], E[T];
#pragma unroll
        for (int k = 0; k < T; ++k) {
            const int r = pass * L * T + gl * T + k;
            qidx[k] = (r < q.len ? (int)codes[q.off + r] : SW_PAD_ROW) * SW_TSTRIDE;
            H[k] = 0; E[k] = 0;
        }
        int diag = 0, mine = 0, nsub = 0;                                // H[row0 - 1][j - 1]; the subject's maximum in this strip; markers seen
        int o_c = SW_MARK, o_h = 0, o_f = 0;                             // what the lane below reads at the next step
        int cur_c = lane < len ? (int)sp[lane] : SW_MARK, nxt_c = SW_MARK;
        int2 cur_l = make_int2(0, 0), nxt_l = make_int2(0, 0);
        if (!first && lane < len) cur_l = lb[lane];
        for (int s = 0; s < nsteps; ++s) {
            const int sl = s & 63;
            if (sl == 0) {                                               // the batch after this one
                const int p = s + 64 + lane;
                nxt_c = p < len ? (int)sp[p] : SW_MARK;
                if (!first) nxt_l = p < len ? lb[p] : make_int2(0, 0);
            }
            const int c0 = __builtin_amdgcn_readlane(cur_c, sl);
            const int h0 = first ? 0 : __builtin_amdgcn_readlane(cur_l.x, sl), f0 = first ? 0 : __builtin_amdgcn_readlane(cur_l.y, sl);
            if (sl == 63) { cur_c = nxt_c; cur_l = nxt_l; }
            int c = lane_up(o_c), hu = lane_up(o_h), fu = lane_up(o_f);
            if (gl == 0) { c = c0; hu = h0; fu = f0; }
            const bool mark = c >= SW_MARK;
            const int extc = mark ? SW_BIG : run.ext, oec = mark ? SW_BIG : run.oe, sadd = mark ? -SW_BIG : 0;
            const int hin = hu;
            int d = diag, h = hu, f = fu;
            diag = mark ? 0 : hu;
            const int8_t *tc = tab + c;
#pragma unroll
            for (int k = 0; k < T; ++k) {
                f = max(f - extc, h - oec);
                const int e = max(E[k] - extc, H[k] - oec);
                h = max(max(d + (int)tc[qidx[k]] + sadd, 0), max(e, f));
                d = H[k]; H[k] = h; E[k] = e;
                mine = max(mine, h);
            }
            o_c = c; o_f = f;
            o_h = mark ? max(hin, mine) : h;
            mine = mark ? 0 : mine;
            if (gl == L - 1) {
                const int j = s - (L - 1);
                if (j >= 0 && j < len) {                                 // a real stream position has reached the last lane
                    if (!last) lb[j] = make_int2(o_h, o_f);
                    else if (mark) {
                        const int pos = sub_pos[ch.sub0 + nsub];
                        const unsigned long long key = ((unsigned long long)(unsigned)o_h << 32) | (0xFFFFFFFFull - (unsigned)pos);
                        kbest = key > kbest ? key : kbest;
                        if (dbg && have) dbg[(long long)q.index * run.dbg_ld + pos] = o_h;
                        ++nsub;
                    }
                }
            }
        }
        if (!last) __threadfence();                                      // the line buffer's writes before the next pass's reads
    }
    if (gl == L - 1 && have && kbest) atomicMax(best + (long long)q.index * run.G + ch.genome, kbest);
}

void launch_sw_score(int cls, const SwQuery *queries, const SwChunk *chunks, int nchunks, const SwRun &run, const uint8_t *codes, const uint8_t *stream,
                     const int *sub_pos, const int8_t *table, int2 *linebuf, unsigned long long *best, int *dbg, hipStream_t s) {
    if (run.nq <= 0 || nchunks <= 0) return;
    const int gpb = SW_THREADS / SW_LANES[cls];
    const dim3 grid((unsigned)((run.nq + gpb - 1) / gpb), (unsigned)nchunks), block(SW_THREADS);
    if (cls == 0) hipLaunchKernelGGL(k_sw_score<16>, grid, block, 0, s, queries, chunks, run, codes, stream, sub_pos, table, linebuf, best, dbg);
    else if (cls == 1) hipLaunchKernelGGL(k_sw_score<32>, grid, block, 0, s, queries, chunks, run, codes, stream, sub_pos, table, linebuf, best, dbg);
    else hipLaunchKernelGGL(k_sw_score<64>, grid, block, 0, s, queries, chunks, run, codes, stream, sub_pos, table, linebuf, best, dbg);
}

}  // namespace pml
