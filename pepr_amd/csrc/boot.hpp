// boot.hpp -- the draw rule of the column bootstrap (include/peprml.h, pml_bootstrap2) as ONE set of functions, compiled for the
// device (k_boot_count, boot.hip) and for the host (pml_boot_draws_host, boot_host.cpp): the two cannot disagree.  Plain C++
// outside hipcc; no HIP include.
//
// Column space of a selection of genes, in selection order (k_gather's layout): L = sum of nsites, P = sum of npat (patterns are
// compressed per gene, never across genes); column c of gene g with local site s has pattern id off_g + site2pat_g[s].
// Replicate r of a call with `seed`: key K_r = gs_mix64(gs_base(seed) + r); draw j (0 <= j < L) is the column
// c_j = gs_draw(K_r, j, L), the multiply-shift rule of genesteps.hpp and rell.hip.  count[r][p] = #{j : pat(c_j) = p}; the
// replicate is the patterns with count > 0 in ascending p, each with weight count[r][p].
// The draws are the project's own (RAxML's -x stream lives inside its binary): parity unpinned.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "genesteps.hpp"

namespace pml {

constexpr int BOOT_TILE = 256;             // patterns k_boot_index compacts per step of its scan (one per thread)
constexpr int BOOT_LDS_BINS = 8192;        // k_boot_count keeps its histogram in LDS (32 KB) up to this many patterns
constexpr int BOOT_CHUNK = 16384;          // draws one workgroup of k_boot_count makes
constexpr int BOOT_MAX_REPS = 65535;       // replicates of one sub-batch: the kernels put the replicate on grid.y

PML_GS_HD uint64_t boot_key(uint64_t seed, uint32_t rep) { return gs_mix64(gs_base(seed) + rep); }
PML_GS_HD uint32_t boot_draw(uint64_t key, uint32_t j, uint32_t L) { return gs_draw(key, j, L); }

// ---- host half (boot_host.cpp) ----
// L of a selection, or -1 with err filled: a gene without columns is fine, L < 1 and L >= 2^31 are refused
long long boot_total_columns(int nsel, const long long *nsites, std::string &err);
// the L columns replicate `rep` draws, in draw order
void boot_draw_columns(unsigned long long seed, int rep, uint32_t ncols, uint32_t *cols_out);
// count[P] of one replicate from the columns' pattern ids col2pat[L] (what k_boot_count computes)
void boot_counts_host(unsigned long long seed, int rep, const std::vector<int> &col2pat, int npat, std::vector<uint32_t> &count);
// the ascending pattern ids with count > 0 (what k_boot_index computes)
void boot_compact_host(const std::vector<uint32_t> &count, std::vector<int> &idx);
// the stepwise-addition seeds of the call's parsimony trees, as jackknife_parsimony_seeds: which 0 = the best tree, 1 + r =
// replicate r; 0 ("input order" to the core) is replaced
unsigned boot_parsimony_seed(unsigned long long seed, int which);

}  // namespace pml
