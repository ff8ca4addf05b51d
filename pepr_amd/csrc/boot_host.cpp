// boot_host.cpp -- the host half of the column bootstrap (boot.hpp): the selection's column count and its refusals, the draws of a
// replicate from the functions the kernel runs, and the counts and the compaction restated on the host.  Plain C++, no HIP: it is
// also built alone under the host sanitizers (tests/boot_standalone).
#include "../../include/peprml.h"
#include "boot.hpp"

namespace pml {

long long boot_total_columns(int nsel, const long long *nsites, std::string &err) {
    if (nsel < 1 || !nsites) { err = "no genes selected"; return -1; }
    long long L = 0;
    for (int i = 0; i < nsel; ++i) {
        if (nsites[i] < 0) { err = "a gene has a negative column count"; return -1; }
        L += nsites[i];
        if (L >= (1ll << 31)) { err = "the concatenation has 2^31 columns or more"; return -1; }
    }
    if (L < 1) { err = "the concatenation has no columns"; return -1; }
    return L;
}

void boot_draw_columns(unsigned long long seed, int rep, uint32_t ncols, uint32_t *cols_out) {
    const uint64_t K = boot_key(seed, (uint32_t)rep);
    for (uint32_t j = 0; j < ncols; ++j) cols_out[j] = boot_draw(K, j, ncols);
}

void boot_counts_host(unsigned long long seed, int rep, const std::vector<int> &col2pat, int npat, std::vector<uint32_t> &count) {
    const uint32_t L = (uint32_t)col2pat.size();
    const uint64_t K = boot_key(seed, (uint32_t)rep);
    count.assign((size_t)npat, 0u);
    for (uint32_t j = 0; j < L; ++j) ++count[(size_t)col2pat[boot_draw(K, j, L)]];
}

void boot_compact_host(const std::vector<uint32_t> &count, std::vector<int> &idx) {
    idx.clear();
    for (size_t p = 0; p < count.size(); ++p) if (count[p]) idx.push_back((int)p);
}

unsigned boot_parsimony_seed(unsigned long long seed, int which) {
    const unsigned s = (unsigned)(seed + (unsigned long long)which);
    return s ? s : 0x9E3779B9u;
}

}  // namespace pml

extern "C" int pml_boot_draws_host(unsigned long long seed, int rep, long long ncols, unsigned *cols_out) {
    if (!cols_out || rep < 0 || ncols < 1 || ncols >= (1ll << 31)) return PML_EINVAL;
    pml::boot_draw_columns(seed, rep, (uint32_t)ncols, cols_out);
    return PML_OK;
}
extern "C" int pml_boot_tile(void) { return pml::BOOT_TILE; }
