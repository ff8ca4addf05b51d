// host.hpp -- host-side model / alignment / tree types of libpeprml (no device code here).
#pragma once
#include <array>
#include <cstdint>
#include <string>
#include <vector>

namespace pml {

constexpr double TMIN = 1.0e-6;     // RAxML 7.2.5 zmax = 1 - 1e-6
constexpr double TMAX = 34.5;       // RAxML 7.2.5 zmin = 1e-15
constexpr double ALPHA_MIN = 0.02;
constexpr double ALPHA_MAX = 1000.0;

struct Model {
    double pi[20];
    double Q[400];
    double eval[20];
    double U[400];      // P(t) = U diag(exp(eval t)) Uinv
    double Uinv[400];
    void init(int pi_mode);
    void init_pi(const double *pi20);    // WAG exchangeabilities with the given frequencies (PROTGAMMAWAGF)
    // any reversible matrix: 190 exchangeabilities (lower triangle by rows, ARNDCQEGHILKMFPSTWYV) and 20 frequencies
    void init(const double *exch190, const double *pi20);
};
const double *wag_exch();                // the built-in 190 exchangeabilities
const double *wag_pi(int pi_mode);       // and the frequencies Model::init(pi_mode) uses (not normalised)
bool parse_paml(const char *text, double *exch190, double *pi20, std::string &err);
struct EncodedAlignment;
// empirical amino-acid frequencies, RAxML's "F" models (spec: oracle/pml_oracle.c po_empirical_freqs)
void empirical_freqs(const EncodedAlignment &a, double *pi20);
// the same scheme from the weighted histogram of the 23 codes alone (every sweep is a function of hist[code]): what a
// device-gathered replicate, whose code matrix exists only in HBM, is counted with (freq.hip k_codehist)
void empirical_freqs_from_counts(const long long *hist23, double *pi20);

// mean rates of K equal-probability Gamma(alpha, mean 1) bins (Yang 1994); K==1 -> {1}
void gamma_rates(double alpha, int K, double *rates);

int aa_code(int ch);                 // 0..19, 20 = B, 21 = Z, 22 = gap/unknown

// A tree's branch lengths: everybody reads them, only Tree's writers below change them, and every change gives the tree a new
// LENGTH STAMP (Tree::len_stamp), unique in the process.  A copy of a tree carries the stamp of the lengths it copies, so two
// trees with equal stamps have equal lengths -- after an assignment, an undo from a backup or a replaced tree as well.  A
// recorded scoring plan compares stamps instead of bytes (Batch::replay_plan).  Code that writes `T.len[v][k] = x` does not compile.
unsigned long long next_len_stamp();           // host.cpp: never 0, never repeated
class BranchLengths {
    std::vector<std::array<double, 3>> v;
    friend struct Tree;
public:
    const std::array<double, 3> &operator[](size_t i) const { return v[i]; }
    size_t size() const { return v.size(); }
    std::vector<std::array<double, 3>>::const_iterator begin() const { return v.begin(); }
    std::vector<std::array<double, 3>>::const_iterator end() const { return v.end(); }
    const std::vector<std::array<double, 3>> &values() const { return v; }
};
struct Tree {
    int ntax = 0;
    std::vector<std::array<int, 3>> nbr;       // -1 = unused (tips use slot 0 only)
    BranchLengths len;
    unsigned long long len_stamp = 0;          // 0: no lengths yet
    int nnodes() const { return (int)nbr.size(); }
    int slot(int v, int w) const { for (int k = 0; k < 3; ++k) if (nbr[v][k] == w) return k; return -1; }
    // the writers of len: one directed slot, all slots cleared, all slots through f, both directions of a branch
    void put_len(int v, int k, double l) { len.v[v][k] = l; len_stamp = next_len_stamp(); }
    void reset_len(size_t nnodes) { len.v.assign(nnodes, {0.0, 0.0, 0.0}); len_stamp = next_len_stamp(); }
    template <class F> void map_len(F f) { for (auto &l : len.v) for (double &x : l) x = f(x); len_stamp = next_len_stamp(); }
    void set_len(int u, int v, double l) { put_len(u, slot(u, v), l); put_len(v, slot(v, u), l); }
    double length() const;
    // names[i] is the label of tip i; returns false and fills err on failure
    static bool parse(const char *newick, const std::vector<std::string> &names, Tree &out, std::string &err);
    // parse without an alignment: tips numbered in order of appearance, names returned
    static bool parse_free(const char *newick, std::vector<std::string> &names, Tree &out, std::string &err);
    std::string newick(const std::vector<std::string> &names, int digits) const;
    // labels[v] (v >= ntax) is printed after the ')' of inner node v when >= 0 (support values);
    // the label belongs to the branch between v and its parent in the printed orientation; digits < 0: no lengths, `)87`
    std::string newick_labeled(const std::vector<std::string> &names, int digits, const std::vector<std::vector<int>> &edge_label) const;
    // same with real-valued labels printed with label_digits decimals (FastTree's 0-1 supports); < 0 = no label
    std::string newick_labeled(const std::vector<std::string> &names, int digits, const std::vector<std::vector<double>> &edge_label, int label_digits) const;
};

// The Newick text as it stands, before Tree binarises it: node 0 is the root, a node's children in text order, parents before
// children; haslen = the node carries ":length"; label = a leaf's name or an inner node's support text.  Same grammar as
// Tree::parse (quotes, [..] comments, optional ';').  treecmp.cpp compares trees that keep their multifurcations.
struct RawNode { std::vector<int> kids; double len = 0; bool haslen = false; std::string label; };
bool parse_newick_raw(const char *newick, std::vector<RawNode> &nodes, std::string &err);

int rf_distance(const Tree &a, const Tree &b);    // (|A|+|B|-2|A&B|)/2 over non-trivial splits
// counts[u][k] = number of `others` containing the bipartition of main's internal edge (u, nbr[u][k]); -1 elsewhere
std::vector<std::vector<int>> support_counts(const Tree &main, const std::vector<Tree> &others);
// The same table from support trees given as Newick TEXT that may cover other taxon sets than main's, under one of three rules:
//   SUPPORT_EQUAL_TAXA  a tree counts only if its leaf set is main's (pml_jackknife's rule; any other tree supports nothing)
//   SUPPORT_DECORATOR   TreeSupportDecorator.addSupportValues (:86-163) on these strings: every node of every support tree,
//                       as rooted in its text after BasicTree.unroot() (:669-717), adds Bipartition(descendant leaves found
//                       among main's sorted taxa, taxon count) (Bipartition.java:41-64: complement over MAIN's taxa, smaller
//                       side by cardinality, on a tie the side holding the lowest index) to a multiset; an edge's count is
//                       the multiset count of its own bipartition.  Depends on where a subset tree's text is rooted.
//   SUPPORT_RESTRICTED  a tree with taxon set S supports main's split A|B if A&S and B&S hold >= 2 taxa each and the tree has
//                       the split A&S | B&S: independent of the rooting of any text
// For trees over main's taxon set the three rules give the same counts.  false + err: a support text does not parse.
enum { SUPPORT_EQUAL_TAXA = 0, SUPPORT_DECORATOR = 1, SUPPORT_RESTRICTED = 2 };
bool support_counts_rule(const Tree &main, const std::vector<std::string> &main_names, const std::vector<const char *> &support,
                         int rule, std::vector<std::vector<int>> &counts, std::string &err);

// PhylogeneticTreeRefiner.getNextIndexToRefine / AdvancedTree.getMeanDescendantSupportValues on a rooted
// support-labelled Newick: ingroup = comma-joined sorted leaves of the next clade to refine ("" = none);
// done = clades already refined (same format); mean_support per node in order of appearance
bool refine_query(const char *newick, int cutoff, const std::vector<std::string> &done, std::string &ingroup,
                  std::vector<int> &mean_support, std::string &err);

struct EncodedAlignment {
    int ntax = 0, nsites = 0, npat = 0, mpad = 0;
    std::vector<std::string> names;
    std::vector<uint8_t> codes;     // [ntax][mpad], padding = gap code
    std::vector<double> weight;     // [mpad], padding = 0
    std::vector<int> site2pat;      // [nsites]
    // rows: ntax pointers to nsites chars; identical columns are merged (first-occurrence order)
    bool encode(int ntax, int nsites, const char *const *names, const char *const *rows, std::string &err);
};

// a constrained split over the gene's taxa: side '1' and side '0' as bitsets ('-' taxa in neither)
struct Constraint { std::vector<uint64_t> one, zero; };
// X (bitset of a cluster / clade) is compatible with the split: misses one side or contains one side
bool split_compatible(const Constraint &c, const std::vector<uint64_t> &X);
bool compatible_with_all(const std::vector<Constraint> &cs, const std::vector<uint64_t> &X);
// leaf sets of all directed messages: L[(v-ntax)*3+k] = taxa on v's side of edge (v, nbr[v][k])
std::vector<std::vector<uint64_t>> leaf_sets(const Tree &t);
bool tree_displays(const Tree &t, const std::vector<Constraint> &cs);
// the non-trivial columns of a FastTree -constraints matrix (ntax named rows of ncons chars '0' '1' '-') over `taxa` (search.cpp)
std::vector<Constraint> constraints_for(const std::vector<std::string> &taxa, int ncons, int ntax, const char *const *names, const char *const *rows);

// The candidate regraft edges of one SPR prune, in the order the search scores them (search.cpp spr_round and the door
// pml_debug_spr_enumerate share this one function).  The prune (p, ks) cuts the subtree behind p's neighbour s = nbr[p][ks]
// off; p's other neighbours x, y (slot order) are joined.  From each inner end of the joined edge (x first) the pruned tree is
// walked depth first, children in slot order; an edge (g, h), h away from the pruning point, has `distance` = the number of
// edges from the joined edge to it, itself included.  Candidates are the edges with rmin <= distance <= rmax; a tip edge is a
// candidate and is not descended.  Constraints: an edge whose far-side leaves joined with the pruned leaves are incompatible
// with a constrained split is no candidate, and nothing behind it is.
// steps = the path CLVs (towards the candidate, one per depth) that have to be built before this candidate and after the
// previous one: depth 0 joins the far end `from` of the joined edge (length tx + ty) with `sib` across `at`; depth d > 0
// carries the path CLV of depth d - 1 across (from, at) and joins it with `sib`.
struct SprStep { int depth, from, at, sib; };
// chain = all `distance` path CLVs from the joined edge to this candidate (what builds its path CLV from nothing)
struct SprCandidate { int g, h, distance; std::vector<SprStep> steps, chain; };
void spr_candidates(const Tree &T, const std::vector<Constraint> &cons, int p, int ks, int rmin, int rmax, std::vector<SprCandidate> &out);

// NJ start tree; with constraints only joins whose cluster is compatible with every split are made
Tree nj_tree(const EncodedAlignment &a, const std::vector<Constraint> *cons = nullptr);
// the two halves of nj_tree: exact integer pair counts ([n*n]: comparable columns, differing columns), and
// Kimura distances + neighbour joining from such counts
void pair_counts(const EncodedAlignment &a, std::vector<int64_t> &cmp, std::vector<int64_t> &diff);
Tree nj_from_counts(int n, const std::vector<int64_t> &cmp, const std::vector<int64_t> &diff, const std::vector<Constraint> *cons = nullptr);

// resumable Brent minimiser on a fixed interval (same control flow as the oracle's eng_opt_alpha)
// FastTree's Gamma20 discretisation (FastTree 2.1 GammaLogLk): 20 fixed rates 0.05 * 400^(k/19);
// weight of rate k = P(mult * hi_k; alpha) - P(mult * lo_k; alpha) for a Gamma(shape alpha, mean 1) rate distribution,
// bin edges at the arithmetic midpoints of adjacent rates (first bin from 0, last to infinity)
void g20_rates(double *rates20);
void g20_weights(double alpha, double mult, double *w20);

struct Brent {
    double a, b, x, w, v, fx, fw, fv, d, e, u, tol = 1e-4;
    int iter; bool done;
    void start(double lo, double hi, double x0, double fx0, double tol_ = 1e-4);
    bool propose();            // sets u; returns false when converged
    void update(double fu);
};

}  // namespace pml
