// msa.hpp -- what the multiple alignment's host rule (msa_host.cpp), its device driver (msa.cpp) and its kernels (msa.hip) share:
// the class geometry, the resolved options, the guide tree, the bound and the host half of a profile alignment.  The rule is in
// include/peprml.h ("Multiple alignment").  Plain C++ outside hipcc; no HIP include.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

struct pml_msa_opts;
struct pml_msa_set;
struct pml_msa_result;

namespace pml {

constexpr int MSA_CLASSES = 3;
constexpr int MSA_STRIP = 8;                     // T: consecutive columns of X a lane keeps in registers; 4 bits a cell = one dword
constexpr int MSA_LANES[MSA_CLASSES] = {16, 32, 64};   // lanes of a group; the widest class takes any LX in passes of 64 x T
constexpr int MSA_THREADS = 64;                  // a workgroup is one wavefront: 64 / lanes merges
constexpr int MSA_GAP = 23;                      // a gap cell of a profile's rows (residue codes are 0 .. 22)
constexpr int MSA_CW = 24;                       // int16 per column of a count profile and of V: 23 codes and a zero
constexpr int MSA_NEG = -(1 << 30);              // minus infinity (peprml.h says why it is low enough)
constexpr int MSA_SCORE_GROUP = 96;              // sequences of consecutive sets whose pair scores share one call of the search's driver
constexpr int MSA_MAX_NX = 32767, MSA_MAX_NY = 255;    // counts and V_j (255 x 128) fit int16

struct MsaOpts { int open, ext, maxabs; int table[576]; };
// false with a message: a negative cost, a table entry outside int8
bool msa_resolve(const pml_msa_opts *o, MsaOpts &r, std::string &err);

// an alignment as codes: row r at rows[r * L], MSA_GAP in a gap cell
struct MsaProfile { int n = 0, L = 0; std::vector<uint8_t> rows; };

struct MsaMerge { int x, y, level; };            // cluster ids (lowest member index), x < y
// the n - 1 merges of a set from S[a * n + b], a < b
void msa_guide_tree(int n, const long long *S, std::vector<MsaMerge> &merges);
// empty, or why the merge is refused: the int32 bound, or counts beyond int16
std::string msa_refusal(int nX, int nY, int LX, int LY, const MsaOpts &o);
// the rule's DP and traceback in plain loops: the score and the path (per merged column 0 = both, 1 = Y's only, 2 = X's only)
long long msa_profile_align_rule(const MsaProfile &X, const MsaProfile &Y, const MsaOpts &o, std::vector<uint8_t> &path);
void msa_merge_rows(const MsaProfile &X, const MsaProfile &Y, const std::vector<uint8_t> &path, MsaProfile &out);

// a call's sets, encoded: sequence k of set s is seq[set_off[s] + k]
struct MsaInput {
    std::vector<int> set_off;                    // [nsets + 1]
    std::vector<long long> off;                  // [nseq + 1] into codes
    std::vector<uint8_t> codes;
    int len(int q) const { return (int)(off[(size_t)q + 1] - off[(size_t)q]); }
};
bool msa_encode_sets(int nsets, const pml_msa_set *sets, MsaInput &in, std::string &err);
// a profile call's operand: rows of equal length, `-` a gap
bool msa_encode_profile(const pml_msa_set *a, const char *what, MsaProfile &p, std::string &err);

// per set: the tree, then every cluster's member order, so that the final rows go back to input order
struct MsaPlan {
    std::vector<MsaMerge> merges;
    std::vector<long long> score;                // per merge
};
// results[s] from the final cluster's rows (in cluster order `members`): rows to input order as text
int msa_fill_result(pml_msa_result *res, const MsaProfile &final_rows, const std::vector<int> &members, const MsaPlan &plan, const std::vector<uint8_t> *path);
// the member order of every cluster after the merges: order[id] (X's members, then Y's)
void msa_member_orders(int n, const std::vector<MsaMerge> &merges, std::vector<std::vector<int>> &order);

}  // namespace pml
