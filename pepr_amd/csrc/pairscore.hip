// pairscore.hip -- the pair scores of the reference's `nj` method (SequenceAlignment.getPairwiseScores, :1042-1067) on the device.
//
// S[i][j] = sum_k table[c_i(k)][c_j(k)] over the columns of an alignment: ntax^2 x columns look-ups in a 24 x 24 table.  The
// score of a concatenation is the sum of its genes' scores (a taxon a gene lacks is a row of '?', which scores 0), so the
// per-gene matrices are computed once (k_pairscore, all genes of a call in one launch) and every replicate of the gene-wise
// jackknife is an integer sum over its genes (k_pairscore_sum).  All sums are integers: nothing depends on the order of the
// atomic adds.
//
// k_pairscore
//   grid    (16 x 16 tile of ordered taxon pairs, chunk of sites, gene); workgroups past a gene's tiles or sites leave at once
//   thread  one ordered pair (i, j) of the tile
//   LDS     the table as int8[24][32] (768 B); per stage of PS_STAGE sites the 16 + 16 code rows of the tile, staged with
//           16-byte loads (rows are 16-byte aligned: ld is a multiple of 16); a row's stride is PS_STAGE + 16 bytes, so the
//           four rows a wavefront reads as i-side words fall into different banks; the table look-ups conflict at random
//   sums    int32 per pair and chunk (a chunk is at most PS_MAX_CHUNK sites of |entry| <= 128), then ONE 64-bit integer
//           global atomic add per pair and chunk
// Every ordered pair is computed, so an asymmetric table is right by construction (no triangle-plus-mirror shortcut).
#include "kernels.h"

namespace pml {

static_assert((long long)PS_MAX_CHUNK * 128 < (1LL << 31), "a chunk's sum of int8 table entries must fit the int32 accumulator");
static_assert(PS_STAGE % 16 == 0 && PS_CHUNK_DEFAULT % 16 == 0 && PS_CHUNK_DEFAULT <= PS_MAX_CHUNK, "stages and chunks start on 16-byte boundaries");
static_assert(PS_CODES * PS_TSTRIDE % 4 == 0 && PS_CODES * PS_TSTRIDE / 4 <= 256, "one thread copies one word of the table");
constexpr int PS_ROW = PS_STAGE + 16;          // LDS stride of a staged row

__global__ __launch_bounds__(256) void k_pairscore(const PairScoreReq *__restrict__ reqs, const int8_t *__restrict__ table, int tiles_max, int chunk_sites) {
    __shared__ __attribute__((aligned(16))) uint8_t rows[2][PS_TILE][PS_ROW];
    __shared__ __attribute__((aligned(16))) int8_t tab[PS_CODES * PS_TSTRIDE];
    const PairScoreReq r = reqs[blockIdx.z];
    const int tiles = (r.ntax + PS_TILE - 1) / PS_TILE;
    const int bi = blockIdx.x / tiles_max, bj = blockIdx.x % tiles_max;
    const long long base = (long long)blockIdx.y * chunk_sites;
    if (bi >= tiles || bj >= tiles || base >= r.nsites) return;          // whole workgroup
    const int tid = threadIdx.x, ti = tid >> 4, tj = tid & 15;
    const int i = bi * PS_TILE + ti, j = bj * PS_TILE + tj;
    const bool active = i < r.ntax && j < r.ntax;
    const int chunk_end = (int)(base + chunk_sites < (long long)r.nsites ? base + chunk_sites : (long long)r.nsites);
    if (tid < PS_CODES * PS_TSTRIDE / 4) ((uint32_t *)tab)[tid] = ((const uint32_t *)table)[tid];
    int acc = 0;
    for (int s0 = (int)base; s0 < chunk_end; s0 += PS_STAGE) {
        const int len = chunk_end - s0 < PS_STAGE ? chunk_end - s0 : PS_STAGE;
        for (int v = tid; v < 2 * PS_TILE * (PS_STAGE / 16); v += 256) {
            const int side = v / (PS_TILE * (PS_STAGE / 16)), row = (v / (PS_STAGE / 16)) % PS_TILE, q = v % (PS_STAGE / 16);
            const int taxon = (side ? bj : bi) * PS_TILE + row;
            // q * 16 < len <= nsites - s0 and ld >= nsites is a multiple of 16, as is s0: the 16 bytes lie inside the row
            if (taxon < r.ntax && q * 16 < len)
                *(uint4 *)&rows[side][row][q * 16] = *(const uint4 *)(r.codes + (size_t)taxon * r.ld + s0 + q * 16);
        }
        __syncthreads();
        if (active) {
            const uint8_t *ri = rows[0][ti], *rj = rows[1][tj];
            int k = 0;
            for (; k + 4 <= len; k += 4) {
                const uint32_t a = *(const uint32_t *)(ri + k), b = *(const uint32_t *)(rj + k);
                acc += tab[(a & 255u) * PS_TSTRIDE + (b & 255u)];
                acc += tab[((a >> 8) & 255u) * PS_TSTRIDE + ((b >> 8) & 255u)];
                acc += tab[((a >> 16) & 255u) * PS_TSTRIDE + ((b >> 16) & 255u)];
                acc += tab[(a >> 24) * PS_TSTRIDE + (b >> 24)];
            }
            for (; k < len; ++k) acc += tab[ri[k] * PS_TSTRIDE + rj[k]];
        }
        __syncthreads();
    }
    if (active) atomicAdd((unsigned long long *)(r.out + (size_t)i * r.ntax + j), (unsigned long long)(long long)acc);
}

__global__ __launch_bounds__(256) void k_pairscore_sum(const PairSumReq *__restrict__ reqs, const long long *const *__restrict__ S,
                                                       const int *__restrict__ gene_ntax) {
    const PairSumReq r = reqs[blockIdx.y];
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= (long long)r.nu * r.nu) return;
    const int i = (int)(p / r.nu), j = (int)(p % r.nu);
    long long sum = 0;
    for (int s = 0; s < r.nsel; ++s) {
        const int li = r.loc[(size_t)s * r.nu + i], lj = r.loc[(size_t)s * r.nu + j];
        if (li < 0 || lj < 0) continue;              // the gene lacks one of the two taxa: a row of '?' scores 0
        const int g = r.sel[s];
        sum += S[g][(size_t)li * gene_ntax[g] + lj];
    }
    r.out[p] = sum;
}

void launch_pairscore(const PairScoreReq *reqs, int nreqs, int max_ntax, int max_nsites, int chunk_sites, const int8_t *table, hipStream_t s) {
    if (nreqs <= 0 || max_ntax <= 0 || max_nsites <= 0) return;
    const int tiles = (max_ntax + PS_TILE - 1) / PS_TILE, chunks = (max_nsites + chunk_sites - 1) / chunk_sites;
    hipLaunchKernelGGL(k_pairscore, dim3((unsigned)(tiles * tiles), (unsigned)chunks, (unsigned)nreqs), dim3(256), 0, s, reqs, table, tiles, chunk_sites);
}

void launch_pairscore_sum(const PairSumReq *reqs, int nreqs, int max_nu, const long long *const *S, const int *gene_ntax, hipStream_t s) {
    if (nreqs <= 0 || max_nu <= 0) return;
    const long long pairs = (long long)max_nu * max_nu;
    hipLaunchKernelGGL(k_pairscore_sum, dim3((unsigned)((pairs + 255) / 256), (unsigned)nreqs), dim3(256), 0, s, reqs, S, gene_ntax);
}

}  // namespace pml
