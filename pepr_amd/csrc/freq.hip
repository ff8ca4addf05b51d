// freq.hip -- k_codehist: the weighted histogram of the 23 residue codes of device-gathered replicates.
//
// A replicate of the gene-wise jackknife is a concatenation of genes that exists only as a code matrix in HBM (k_gather).
// The empirical-frequency scheme of the "F" models and of PROTGAMMAGTR (host.cpp empirical_freqs) needs nothing of that
// matrix but hist[code] = the summed pattern weights of the cells holding the code (empirical_freqs_from_counts), so the
// matrix is counted where it lives: one launch for all replicates of a batch, ntax x mpad bytes read once each.
//
//   grid    (replicate, block of 256 patterns); blocks past a replicate's mpad leave at once
//   thread  one pattern: walks the taxon rows of codes[ntax][mpad] (consecutive threads read consecutive bytes of a row)
//           and adds (long long)weight[p] to the code's bin; padding patterns weigh 0 and the gap rows of absent taxa hold
//           the gap code (k_gather), so both are right by construction
//   bins    8 copies of the 23 bins in LDS (a thread uses copy tid & 7: an eighth of the same-address conflicts), folded and
//           flushed with one 64-bit integer global atomic add per non-empty bin: integer sums, independent of order
#include "kernels.h"

namespace pml {

constexpr int HIST_COPIES = 8;

__global__ __launch_bounds__(256) void k_codehist(const CodeHistReq *__restrict__ reqs, unsigned long long *__restrict__ out) {
    __shared__ unsigned long long bins[HIST_COPIES][NCODES + 1];
    const CodeHistReq r = reqs[blockIdx.x];
    if ((int)blockIdx.y * 256 >= r.mpad) return;                    // whole workgroup: nothing of this replicate here
    const int tid = threadIdx.x, p = blockIdx.y * 256 + tid;
    if (tid < HIST_COPIES * (NCODES + 1)) (&bins[0][0])[tid] = 0;
    __syncthreads();
    if (p < r.mpad) {
        const unsigned long long w = (unsigned long long)(long long)r.weight[p];
        if (w != 0) {
            unsigned long long *mine = bins[tid & (HIST_COPIES - 1)];
            const uint8_t *col = r.codes + p;
            for (int t = 0; t < r.ntax; ++t) {
                const int code = col[(size_t)t * r.mpad];
                atomicAdd(mine + (code < NCODES ? code : NCODES - 1), w);
            }
        }
    }
    __syncthreads();
    if (tid < NCODES) {
        unsigned long long sum = 0;
        for (int c = 0; c < HIST_COPIES; ++c) sum += bins[c][tid];
        if (sum) atomicAdd(out + (size_t)blockIdx.x * NCODES + tid, sum);
    }
}

static_assert(HIST_COPIES * (NCODES + 1) <= 256, "one thread clears one LDS bin");

void launch_codehist(const CodeHistReq *reqs, int nreqs, int max_mpad, long long *out, hipStream_t s) {
    if (nreqs <= 0 || max_mpad <= 0) return;
    hipLaunchKernelGGL(k_codehist, dim3((unsigned)nreqs, (unsigned)((max_mpad + 255) / 256)), dim3(256), 0, s, reqs, (unsigned long long *)out);
}

}  // namespace pml
