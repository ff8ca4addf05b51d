// treecmp.cpp -- the split records of a set of trees, as TreeComparison sees them (host only; the kernels are treecmp.hip, the
// C ABI treecmpapi.cpp).  What the Java does with a text, and where (restated in tests/treecmp_ref.py):
//   BasicTree.parseNewickTreeString (BasicTree.java:131-409) numbers the leaves in text order and the inner nodes in the order
//     of their ')'; a branch without a length has length 0 (:286); an inner node's label is its support (:313-323) and plays
//     no part in any value here.
//   getTreeString(useLengths, true) (:450-520) prints a node's children in ascending node index (populateChildPointers
//     :438-447): its leaves first, then its inner children; without useLengths no length is printed, so every length is 0.
//   TreeParser.parseTreeString (TreeParser.java:26-175) on that text: one TreeBranch per node that is neither the root nor a
//     child of the root, in ascending node index (:83-110), pendant branches included; then two top-level nodes become ONE
//     branch whose length is the sum of the two (:138-151), three become three branches to a new node (:152-162); any other
//     number leaves no tree (:163-172; refused here).
//   A node with one child is printed without parentheses (:493, :509), which makes "A:1:2" of its leaf: the name no longer
//     matches any other tree's.  Refused here.
//   Tree.getBranches() (Tree.java:249-253) is HashSet.toArray over objects without hashCode: the Java's order is the JVM's
//     identity-hash order and differs from run to run.  This project pins the order of creation above.
#include <algorithm>
#include <limits>
#include <unordered_map>

#include "../../include/peprml.h"
#include "host.hpp"
#include "treecmp.hpp"

namespace pml {

namespace {
struct Bits {
    int W; std::vector<unsigned long long> w;
    Bits(int W_, size_t nodes) : W(W_), w(nodes * (size_t)W_, 0) {}
    unsigned long long *at(int v) { return w.data() + (size_t)v * W; }
};

// the normalised words of a side, and whether the split is trivial
bool normalise(const unsigned long long *side, int n, int W, unsigned long long *out) {
    int m = 0;
    for (int k = 0; k < W; ++k) { out[k] = side[k]; m += __builtin_popcountll(side[k]); }
    if (2 * m > n || (2 * m == n && !(out[0] & 1))) {
        for (int k = 0; k < W; ++k) {
            const int bits = n - k * 64;
            out[k] = ~out[k] & (bits >= 64 ? ~0ull : bits > 0 ? (1ull << bits) - 1 : 0);
        }
        m = n - m;
    }
    return m <= 1;
}

int build_one(const char *text, int use_lengths, int t, TcSet &S, std::string &err) {
    const std::string who = "tree " + std::to_string(t) + ": ";
    std::vector<RawNode> nd;
    std::string perr;
    if (!parse_newick_raw(text, nd, perr)) { err = who + perr; return PML_EPARSE; }
    const int N = (int)nd.size();
    if (nd[0].kids.empty()) { err = who + "a single leaf is no tree"; return PML_EINVAL; }
    std::vector<std::string> leaves;
    for (const RawNode &x : nd) {
        if (x.kids.size() == 1) { err = who + "a node with one child (the reference prints it without parentheses and then misreads the leaf's name)"; return PML_EINVAL; }
        if (x.kids.empty()) leaves.push_back(x.label);
    }
    if (nd[0].kids.size() != 2 && nd[0].kids.size() != 3) {
        err = who + "has " + std::to_string(nd[0].kids.size()) + " top level nodes. Only 2 and 3 are valid (TreeParser.java:164)"; return PML_EINVAL;
    }
    {
        std::vector<std::string> sorted = leaves;
        std::sort(sorted.begin(), sorted.end());
        for (size_t i = 1; i < sorted.size(); ++i) if (sorted[i] == sorted[i - 1]) { err = who + "duplicate leaf '" + sorted[i] + "'"; return PML_EINVAL; }
        if (t == 0) {
            if (sorted.size() < 3) { err = who + "need at least 3 taxa"; return PML_EINVAL; }
            if (sorted.size() > (size_t)TC_MAX_TAXA) { err = who + "has " + std::to_string(sorted.size()) + " taxa: a tree comparison takes at most " + std::to_string(TC_MAX_TAXA); return PML_EINVAL; }
            S.names = sorted; S.n = (int)sorted.size(); S.W = tc_words(S.n);
        } else if (sorted != S.names) {
            err = who + "its leaf labels differ from tree 0's (" + std::to_string(sorted.size()) + " against " + std::to_string(S.names.size()) + " leaves, or other names): prune the trees to their common taxa first";
            return PML_EINVAL;
        }
    }
    const int n = S.n, W = S.W;
    std::unordered_map<std::string, int> index;
    for (int i = 0; i < n; ++i) index[S.names[(size_t)i]] = i;
    // leaf sets below every node: children have higher indices than their parent
    Bits below(W, (size_t)N);
    std::vector<int> parent((size_t)N, -1);
    for (int v = N - 1; v >= 0; --v) {
        if (nd[v].kids.empty()) { const int i = index[nd[v].label]; below.at(v)[i >> 6] |= 1ull << (i & 63); }
        for (int c : nd[v].kids) { parent[c] = v; for (int k = 0; k < W; ++k) below.at(v)[k] |= below.at(c)[k]; }
    }
    // the Java's node index after the round trip: children reordered (leaves first, both groups in text order), then leaves
    // in text order and inner nodes in the order of their ')'
    std::vector<int> jleaf, jinner;
    {
        std::vector<std::vector<int>> kids((size_t)N);
        for (int v = 0; v < N; ++v) {
            for (int c : nd[v].kids) if (nd[c].kids.empty()) kids[v].push_back(c);
            for (int c : nd[v].kids) if (!nd[c].kids.empty()) kids[v].push_back(c);
        }
        std::vector<std::pair<int, size_t>> stack{{0, 0}};
        while (!stack.empty()) {
            auto &top = stack.back();
            const int v = top.first;
            if (kids[v].empty()) { jleaf.push_back(v); stack.pop_back(); continue; }
            if (top.second < kids[v].size()) { const int c = kids[v][top.second++]; stack.push_back({c, 0}); }
            else { jinner.push_back(v); stack.pop_back(); }
        }
    }
    TcTree T;
    std::vector<unsigned long long> tmp((size_t)W);
    auto emit = [&](const unsigned long long *side, double length, int flags) {
        const bool trivial = normalise(side, n, W, tmp.data());
        T.words.insert(T.words.end(), tmp.begin(), tmp.end());
        T.len.push_back(length);
        T.flags.push_back(flags | (trivial ? TC_TRIVIAL : 0));
    };
    auto length_of = [&](int v) { return use_lengths && nd[v].haslen ? nd[v].len : 0.0; };
    std::vector<int> order = jleaf;
    order.insert(order.end(), jinner.begin(), jinner.end());
    std::vector<int> top;
    for (int v : order) {
        if (v == 0) continue;
        if (parent[v] == 0) { top.push_back(v); continue; }
        emit(below.at(v), length_of(v), TC_REAL);
    }
    if (top.size() == 2) emit(below.at(top[0]), length_of(top[0]) + length_of(top[1]), TC_REAL);
    else for (int v : top) emit(below.at(v), length_of(v), TC_REAL);
    T.nreal = T.nrec();
    // what Tree::parse adds for a multifurcation below the root: children k0 .. km-1 in TEXT order become a ladder whose inner
    // edges split off k0+k1, k0+k1+k2, ... k0+..+km-2 (host.cpp Builder::build)
    for (int v = 1; v < N; ++v) {
        const auto &k = nd[v].kids;
        if (k.size() < 3) continue;
        std::vector<unsigned long long> acc(below.at(k[0]), below.at(k[0]) + W);
        for (size_t i = 1; i + 1 < k.size(); ++i) {
            for (int w = 0; w < W; ++w) acc[(size_t)w] |= below.at(k[i])[w];
            emit(acc.data(), 0.0, 0);
        }
    }
    // StatisticsUtilities.getMaximum (:194-205) and TreeComparison.java:641-651
    double mx = -std::numeric_limits<double>::infinity();
    for (int b = 0; b < T.nreal; ++b) { const double l = T.len[(size_t)b]; if (l == l) mx = std::max(mx, l); }
    T.maxlen = mx;
    T.lnorm.resize(T.len.size(), 0.0);
    for (int b = 0; b < T.nreal; ++b) T.lnorm[(size_t)b] = T.len[(size_t)b] / mx;
    S.trees.push_back(std::move(T));
    return PML_OK;
}
}  // namespace

int tc_build(int ntrees, const char *const *newicks, int use_lengths, TcSet &out, std::string &err) {
    out = TcSet();
    if (ntrees < 1 || !newicks) { err = "a tree comparison needs at least one tree"; return PML_EINVAL; }
    for (int t = 0; t < ntrees; ++t) {
        if (!newicks[t]) { err = "tree " + std::to_string(t) + ": null text"; return PML_EINVAL; }
        if (int rc = build_one(newicks[t], use_lengths, t, out, err)) return rc;
    }
    return PML_OK;
}

}  // namespace pml
