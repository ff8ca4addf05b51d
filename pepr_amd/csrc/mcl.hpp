// mcl.hpp -- what the Markov clustering path's host rule (mcl_host.cpp), its device driver (mcl.cpp) and its kernels (mcl.hip)
// share: the class limits, the graph front end and the reading of a limit matrix.  The rule is in include/peprml.h ("Homolog
// groups").  Plain C++ outside hipcc; no HIP include.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

struct pml_mcl_opts;

namespace pml {

constexpr int MCL_PACKED_MAX = 16;         // packed class: one wavefront per component, four components per workgroup, one 16 x 16 tile
constexpr int MCL_LDS_MAX = 96;            // LDS class: one workgroup per component, two buffers of 96 columns in LDS
constexpr int MCL_LDS_LD = MCL_LDS_MAX + 2;// their column stride in doubles: 16 lanes 98 doubles apart fall into 16 different bank pairs
constexpr int MCL_TILE = 64;               // k_mcl_expand: a workgroup's tile of C, and the padding of an HBM-class matrix
constexpr int MCL_KSTEP = 16;              // its LDS panels' depth
constexpr int MCL_THREADS = 256;

struct MclOpts { double inflation, prune_inverse, chaos_eps; int max_iter; };
MclOpts mcl_resolve(const pml_mcl_opts *o);
inline int mcl_words(int n) { return (n + 31) / 32; }

// the mirrored graph with its components: nodes renumbered so that a component's nodes are consecutive (ascending by their
// index in the call), components in order of their smallest member.  CSR by column of the renumbered graph; a row index is
// local to its component
struct MclGraph {
    int n = 0;
    std::vector<int> comp_off;             // [ncomp + 1] into nodes
    std::vector<int> nodes;                // [n] the call's node index of renumbered node p
    std::vector<long long> ptr;            // [n + 1]
    std::vector<int> row;                  // local row of every entry
    std::vector<double> val;
    int ncomp() const { return (int)comp_off.size() - 1; }
    int size(int c) const { return comp_off[(size_t)c + 1] - comp_off[(size_t)c]; }
};
// false with a message: an index out of range, a weight that is not finite or <= 0
bool mcl_build_graph(int n, long long narcs, const int *a, const int *b, const double *w, MclGraph &g, std::string &err);
// column-major n x n start matrix of component c (loops, normalised)
void mcl_fill_host(const MclGraph &g, int c, std::vector<double> &M);
// one iteration on a column-major matrix, in place (tmp is scratch); returns chaos
double mcl_step_host(int n, std::vector<double> &M, std::vector<double> &tmp, const MclOpts &o);
// what the kernels leave of a limit matrix: best[j] = the attractor row with the largest M_aj (-1: no attractor), and for every
// attractor column b the bit mask (mcl_words(n) words) of the attractor rows a with M_ab > 0; other columns' masks are 0
void mcl_read_host(int n, const std::vector<double> &M, int *best, unsigned *mask);
// the cluster of every node from the components' best rows and masks (both concatenated component by component; a component's
// masks are size x mcl_words(size) words), numbered in output order
void mcl_finish(const MclGraph &g, const int *best, const unsigned *mask, int *cluster_of, int *nclusters);

// ---- the Java around MCL ----
std::string java_float_to_string(float v);
bool hits_filter(const char *t, size_t n, std::string &out, std::string &err);
void hits_bidirectional(const char *t, size_t n, int score_field, std::string &out);
// `id1 id2 w` lines (fields split at blanks and tabs; a line of fewer than two fields is skipped, a missing weight is 1)
bool abc_parse(const char *t, size_t n, std::vector<std::string> &labels, std::vector<int> &a, std::vector<int> &b, std::vector<double> &w, std::string &err);
void homolog_select(int nclusters, const long long *off, const int *members, const int *taxon_of_node, int min_taxa, int max_taxa, bool rep_only, int target_ntax,
                    int target_min_gene, std::vector<int> &kept);

}  // namespace pml
