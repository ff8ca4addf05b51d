// fitch_dev.hpp -- what the Fitch kernels of parsimony.hip and genesteps.hip share: the state set of an alignment code, the Fitch
// operator, and the segment descriptor of k_fitch_tips with its launch.  hipcc only.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace pml {

// state set of an alignment code (host.hpp aa_code): the one table of the text path and of k_fitch_tips
__host__ __device__ __forceinline__ unsigned code_mask(int c) {
    if (c < 20) return 1u << c;
    if (c == 20) return (1u << 2) | (1u << 3);     // B = N | D
    if (c == 21) return (1u << 5) | (1u << 6);     // Z = Q | E
    return 0xFFFFFu;
}
// one (replicate, gene) segment of k_fitch_tips: patterns [0, npat) of the gene go to [dst_off, dst_off + npat) of the replicate's
// tip rows and weights; rowmap[t] = the gene's row of replicate taxon t, -1 = the gene lacks it.  src == null: the padding
// segment [dst_off, dst_off + npat) = [sum of npat, mpad) of the replicate, every set bit and weight 0
struct FTipSeg {
    const uint8_t *src; const double *w; const int *rowmap; unsigned *pool; int *dst_w;
    int src_mpad, npat, mpad, dst_off, ntax_dst, pad;
};

__device__ __forceinline__ unsigned fitch(unsigned l, unsigned r) { const unsigned x = l & r; return x ? x : (l | r); }

// k_fitch_tips (parsimony.hip) over nsegs segments (device memory) of at most max_npat patterns each
void launch_fitch_tips(const FTipSeg *segs, int nsegs, int max_npat, hipStream_t s);

}  // namespace pml
