// treecmp.hpp -- the host half of the tree-set comparison (treecmp.cpp): plain C++, no HIP, also built alone.
// The model is the one TreeComparison compares (TreeComparison.java:129-136): TreeParser.parseTreeString on the text that
// BasicTree.getTreeString(useLengths, true) prints.  tests/treecmp_ref.py restates it with the Java's file:line.
#pragma once
#include <cmath>
#include <string>
#include <vector>

namespace pml {

constexpr int TC_MAX_TAXA = 512;               // == CG_MAX_TAXA: a split is at most 8 words
constexpr int tc_words(int n) { return n <= 64 ? 1 : n <= 128 ? 2 : n <= 256 ? 4 : 8; }      // == cg_words
// flags of a split record.  TC_LAST is set on the device (k_tree_sort): the record is the last of its tree with its split
enum { TC_REAL = 1 /* a TreeBranch of the Java's tree */, TC_TRIVIAL = 2 /* one side is a single leaf */, TC_LAST = 4 };

// One tree's records.  The first nreal are the tree's TreeBranches in the order TreeParser creates them; behind them come the
// splits that Tree::parse (host.cpp) adds when it resolves a multifurcation into a ladder: they carry no flag and no length and
// serve rf_splits alone, which has to agree with pml_rf_distance.
struct TcTree {
    int nreal = 0;
    std::vector<unsigned long long> words;     // [nrec][W], normalised: the side with fewer leaves, on a tie the side holding taxon 0
    std::vector<double> len, lnorm;            // the branch's length, and length / maxlen
    std::vector<int> flags;
    double maxlen = 0;                         // StatisticsUtilities.getMaximum: -inf when every length is NaN
    int nrec() const { return (int)flags.size(); }
};
struct TcSet {
    std::vector<std::string> names;            // sorted leaf names: taxon i = bit i & 63 of word i >> 6
    int n = 0, W = 1;
    std::vector<TcTree> trees;
};
// PML_OK, PML_EPARSE (a text does not parse) or PML_EINVAL (see peprml.h); err names the tree
int tc_build(int ntrees, const char *const *newicks, int use_lengths, TcSet &out, std::string &err);

// (|union| - |intersection|) / 2 over sets of dA and dB distinct splits that share `shared`; Java int division
inline int tc_rf(long long dA, long long dB, long long shared) { return (int)((dA + dB - 2 * shared) / 2); }
// TreeComparison.java:745 / :808 from the three sums
inline double tc_distance(double r, double ss1, double ss2) { return std::sqrt(r) / std::sqrt(ss1 + ss2); }

}  // namespace pml
