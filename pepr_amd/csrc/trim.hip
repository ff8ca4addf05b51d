// trim.hip -- the reference's `-uniform_trim` (MSATrimmer.trimUniformColumns, :205-253) and MSATrimmer's two sibling filters
// (trimUniformativeColumns :141-203, trimTopologicallyUninformativeColumns :264-351) on the device, in front of the congruence
// filter.  All three decisions fall out of one pass over a column; the rules are trim.hpp's trim_decide.
//
// k_colclass    workgroup = TRIM_COLS columns of one gene, thread = one column.  Every byte of the alignment is read exactly once,
//               so nothing is staged in LDS: for each row a wavefront's 64 adjacent columns are one 64-byte segment.  The thread
//               keeps the set of bytes it has seen and the set it has seen twice as two 256-bit masks in registers (16 VGPRs) and
//               the number of rows that show neither '-' nor '?'; no per-column state grows with the number of rows, so a gene
//               may have any number of them.  It stores one flag byte.  The '-' and '?' cells are summed per wavefront and added
//               to the gene's counter with one 64-bit atomicAdd per wavefront: an integer sum, the order does not matter.
// k_colgather   out[r][j] = in[r][src_col[j]]: thread = one 16-byte chunk of the output row; it holds its 16 source columns in
//               registers and walks down TRIM_ROWS rows, one 16-byte store per row (a wavefront stores 1 KiB contiguously).  The
//               bytes behind the last kept column, up to the row stride, are written as 0.
//
// The kept columns' exclusive prefix is built on the host from the flags (trim.cpp), as the congruence path does with nsplit /
// rec_off: no device scan.  No kernel allocates; no thread waits on another.
#include "kernels.h"
#include "trim.hpp"

namespace pml {

__global__ __launch_bounds__(TRIM_COLS) void k_colclass(const CgGene *__restrict__ genes, const int *__restrict__ tile_gene, const int *__restrict__ tile_first,
                                                        uint8_t *__restrict__ flags, long long *gap_or_missing) {
    const int gi = tile_gene[blockIdx.x];
    const CgGene g = genes[gi];
    const int c = ((int)blockIdx.x - tile_first[gi]) * TRIM_COLS + (int)threadIdx.x;
    const bool active = c < g.ncols;                                   // no early return: every lane takes part in the shuffles
    uint32_t seen1[8] = {0, 0, 0, 0, 0, 0, 0, 0}, seen2[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int shown = 0;
    if (active) {
        const uint8_t *p = g.bytes + c;                                // c < ncols <= ld: inside every row
#pragma unroll 4
        for (int r = 0; r < g.ntax; ++r) trim_note(seen1, seen2, shown, p[(size_t)r * g.ld]);
        flags[g.col_base + c] = (uint8_t)trim_decide(seen1, seen2, shown, g.ntax);
    }
    long long hidden = active ? (long long)(g.ntax - shown) : 0;       // the column's '-' and '?' cells
    for (int off = 32; off > 0; off >>= 1) hidden += __shfl_xor(hidden, off);
    if ((threadIdx.x & 63) == 0 && hidden) atomicAdd((unsigned long long *)&gap_or_missing[gi], (unsigned long long)hidden);
}

__global__ __launch_bounds__(256) void k_colgather(const TgGene *__restrict__ genes, const TgTile *__restrict__ tiles) {
    const TgTile t = tiles[blockIdx.x];
    const TgGene g = genes[t.gene];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = t.chunk0 + lane;                                     // 16-byte chunk of the output row
    if (q * 16 >= g.ld_out) return;                                    // no barrier follows
    int src[16];
#pragma unroll
    for (int v = 0; v < 4; ++v) {                                      // src_col holds ld_out entries: q * 16 + 15 < ld_out
        const int4 s4 = *(const int4 *)(g.src_col + q * 16 + v * 4);
        src[v * 4] = s4.x; src[v * 4 + 1] = s4.y; src[v * 4 + 2] = s4.z; src[v * 4 + 3] = s4.w;
    }
#pragma unroll
    for (int k = 0; k < 16; ++k) if (q * 16 + k >= g.nkept) src[k] = -1;
    const int r1 = t.row0 + TRIM_ROWS < g.ntax ? t.row0 + TRIM_ROWS : g.ntax;
    for (int r = t.row0 + wave; r < r1; r += 4) {
        const uint8_t *row = g.in + (size_t)r * g.ld_in;
        uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const uint32_t at = row[src[k] >= 0 ? src[k] : 0];          // src[k] < the input's ncols <= ld_in; nkept > 0, so column 0 exists
            const uint32_t b = src[k] >= 0 ? at : 0u;
            w[k >> 2] |= b << (8 * (k & 3));
        }
        *(uint4 *)(g.out + (size_t)r * g.ld_out + (size_t)q * 16) = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

void launch_colclass(const CgGene *genes, const int *tile_gene, const int *tile_first, int ntiles, uint8_t *flags, long long *gap_or_missing, hipStream_t s) {
    if (ntiles <= 0) return;
    hipLaunchKernelGGL(k_colclass, dim3((unsigned)ntiles), dim3(TRIM_COLS), 0, s, genes, tile_gene, tile_first, flags, gap_or_missing);
}

void launch_colgather(const TgGene *genes, const TgTile *tiles, int ntiles, hipStream_t s) {
    if (ntiles <= 0) return;
    hipLaunchKernelGGL(k_colgather, dim3((unsigned)ntiles), dim3(256), 0, s, genes, tiles);
}

}  // namespace pml
