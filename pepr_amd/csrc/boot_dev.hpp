// boot_dev.hpp -- descriptors and launches of the bootstrap kernels (boot.hip) and the host objects that drive them (boot.cpp):
// the column space of a gene selection resident on the device, and the counts and compactions of a sub-batch of replicates.
// hipcc only.
#pragma once
#include <hip/hip_runtime.h>

#include "boot.hpp"
#include "engine.hpp"

namespace pml {

// one selected gene: its patterns [0, npat) are the patterns [pat_off, pat_off + npat) of the selection
struct BootSeg { const uint8_t *src; int src_mpad, pat_off, npat, pad; };
// the selection: col2pat[L] = the pattern id of every column, segs[nseg] ascending in pat_off, rowmaps[nseg][ntax] = the gene's
// row of union taxon t or -1
struct BootSpace { const int *col2pat; const BootSeg *segs; const int *rowmaps; unsigned L; int P, nseg, ntax; };
// one replicate of a sub-batch.  count[P], idx[P] and npat_dev are written by k_boot_count / k_boot_index; npat (read back by the
// host), mpad and the destinations are filled in before k_boot_gather / k_boot_pairs run
struct BootRep {
    unsigned long long key; unsigned *count; int *idx; int *npat_dev;
    void *dst; void *dst_w;                 // form 0: uint8 codes [ntax][mpad], f64 weights; form 1: uint32 state sets [ntax][mpad], int weights
    long long *cmp, *diff;                  // [ntax][ntax], zeroed by the host
    int npat, mpad;
};
enum { BOOT_FORM_CODES = 0, BOOT_FORM_MASKS = 1 };

void launch_boot_count(const BootSpace &sp, const BootRep *reps, int nreps, bool global_form, hipStream_t s);
void launch_boot_index(const BootSpace &sp, const BootRep *reps, int nreps, hipStream_t s);
void launch_boot_gather(const BootSpace &sp, const BootRep *reps, int nreps, int max_mpad, int form, hipStream_t s);
void launch_boot_pairs(const BootSpace &sp, const BootRep *reps, int nreps, hipStream_t s);

// The column space of one selection of store genes, built once per call and kept in HBM
struct BootSet {
    Ctx *ctx = nullptr;
    std::vector<std::string> names;         // sorted union of the genes' taxa
    std::vector<int> col2pat;               // the pattern id of every column, as uploaded
    long long L = 0; int P = 0, nseg = 0;
    char *d_buf = nullptr; BootSpace sp{};
    int create(Ctx *c, const GeneStore &store, const std::vector<int> &sel);
    void destroy() { if (d_buf) { hipFree(d_buf); d_buf = nullptr; } }
    ~BootSet() { destroy(); }
};
// count, index and the read-back of npat for replicates [begin, end) of the call with `seed`; then gather and pairs into
// destinations the caller has laid out
struct BootReps {
    Ctx *ctx = nullptr; const BootSet *set = nullptr;
    int n = 0; char *d_buf = nullptr; BootRep *d_reps = nullptr;
    std::vector<BootRep> h; std::vector<int> npat;
    long long *d_pairs = nullptr;           // [n][2][ntax][ntax], after pairs()
    int count_and_index(Ctx *c, const BootSet &s, int begin, int end, unsigned long long seed);
    int gather(int form);                   // h[r].dst, dst_w, mpad set by the caller
    int pairs(std::vector<std::vector<int64_t>> &cmp, std::vector<std::vector<int64_t>> &diff);   // after gather(BOOT_FORM_CODES)
    int read_idx(int r, std::vector<int> &idx);
    void destroy() { if (d_buf) { hipFree(d_buf); d_buf = nullptr; } if (d_pairs) { hipFree(d_pairs); d_pairs = nullptr; } }
    ~BootReps() { destroy(); }
};
// bytes BootReps holds per replicate of a selection with P patterns
inline size_t boot_rep_bytes(int P) { return (size_t)P * 8 + 256; }

}  // namespace pml
