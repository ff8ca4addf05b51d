"""TreeComparison's `-rf` and `-tree_dist` legs restated in Python, with the file:line of the Java each piece restates
(src/edu/vt/vbi/ci/pepr/tree/ of the reference).  Our own code: nothing here is the reference's program text.  Sets are real
Python sets, sums are Python floats (IEEE doubles, one rounding per operation, no fused multiply-add) in the Java's order.

THE TREE MODEL.  TreeComparison compares TreeParser.parseTreeString(BasicTree.getTreeString(useLengths, true))
(TreeComparison.java:129-136).  The answers to the six questions of that model:

 order of getBranches()   NOT DEFINED by the Java.  Tree.getBranches() (Tree.java:249-253) is HashSet.toArray(), the set holds
                          TreeBranch objects (Tree.java:52-64), TreeBranch has neither hashCode nor equals: the order is the
                          JVM's identity-hash order and changes from run to run.  Nothing integer depends on it.  The f64 sums
                          depend on it in their last bits, and with a repeated split the counterpart does.  We pin ONE of the
                          orders the Java can take: the order in which TreeParser creates the TreeBranch objects --
                          (TreeParser.java:83-110) node index ascending, skipping the root and its children, then the
                          top-level branch or branches (:137-162).  Node indices are BasicTree's (BasicTree.java:160-276):
                          leaves in text order, then inner nodes in the order of their ')'; and the text is the ROUND-TRIPPED
                          one, in which getNodeString (:480-520) prints a node's children in ascending node index
                          (populateChildPointers :438-447), i.e. its leaves before its inner children.
 which branches           one per node that is neither the root nor a child of the root, pendant branches included
                          (TreeParser.java:104-109), plus the top level.
 rooted top level (A,B);  ONE branch between A and B whose length is the SUM of the two lengths (TreeParser.java:138-151).  A top
                          level of three gives three branches to a new node (:152-162).  Any other top level: no tree (:163-172,
                          the NullPointerException is caught, parseTreeString returns null and compareAllvsAll skips the pair
                          :272); refused here (ValueError).
 degree-2 node            getNodeString prints a node with one child without parentheses (:493, :509): "((A:1):2,B,C)" becomes
                          "(A:1.0:2.0,B..." and the second parse takes "A:1.0:2.0" for a leaf name (:187-205), which no other
                          tree has.  Refused here (ValueError).
 branch without a length  0.0: BasicTree fills branchLengths with 0 (:286) and getTreeString prints it (":0.0"), so TreeBranch's
                          own default of 1 (TreeBranch.java:11, :51-53) is never reached.  Without useLengths no length is
                          printed and every length is 0.0.
 support label            the text between ')' and ':' is the support of the branch ABOVE that node (BasicTree.java:313-323,
                          printed back at :512-516, TreeParser.java:33-43).  It enters no value computed here (the printing of
                          TreeComparison.java:656-732 is left out).
"""
import math
import sys

import numpy as np

if sys.getrecursionlimit() < 20000:        # a caterpillar of 512 leaves nests 510 deep and every level costs a few frames
    sys.setrecursionlimit(20000)

REAL, TRIVIAL, LAST = 1, 2, 4          # the flags of a split record (include/peprml.h pml_tree_splits)


# ---- Newick text -> nodes (our own reader; BasicTree.parseNewickTreeString's outcome for well-formed text) ----
class Node:
    def __init__(self):
        self.kids, self.name, self.length, self.label = [], None, None, ""

    def is_leaf(self):
        return not self.kids


def parse_newick(text):
    s = text.strip()
    if s.endswith(";"):
        s = s[:-1]
    pos = 0

    def sub():
        nonlocal pos
        nd = Node()
        if s[pos] == "(":
            pos += 1
            while True:
                nd.kids.append(sub())
                if s[pos] == ",":
                    pos += 1
                    continue
                if s[pos] == ")":
                    pos += 1
                    break
                raise ValueError("expected , or ) at %d" % pos)
        b = pos
        while pos < len(s) and s[pos] not in ",():":
            pos += 1
        if nd.kids:
            nd.label = s[b:pos]
        else:
            nd.name = s[b:pos]
            if not nd.name:
                raise ValueError("empty leaf name at %d" % pos)
        if pos < len(s) and s[pos] == ":":
            pos += 1
            b = pos
            while pos < len(s) and s[pos] not in ",()":
                pos += 1
            nd.length = float(s[b:pos])
        return nd

    root = sub()
    if pos != len(s):
        raise ValueError("text after the tree at %d" % pos)
    return root


def leaves_below(nd):
    return [nd.name] if nd.is_leaf() else [x for k in nd.kids for x in leaves_below(k)]


def all_nodes(nd):
    yield nd
    for k in nd.kids:
        yield from all_nodes(k)


# ---- the Tree that TreeComparison compares ----
class Branch:
    """a TreeBranch: its two leaf sets (getBipartitionLeafSets, TreeBranch.java:227-261) and its length"""

    def __init__(self, side0, side1, length):
        self.sides = (frozenset(side0), frozenset(side1))
        self.length = length


class JTree:
    def __init__(self, text, use_lengths=True):
        root = parse_newick(text)
        self.root = root
        self.leaves = leaves_below(root)
        if root.is_leaf():
            raise ValueError("a single leaf is no tree")
        if len(set(self.leaves)) != len(self.leaves):
            raise ValueError("duplicate leaf")
        for nd in all_nodes(root):
            if len(nd.kids) == 1:
                raise ValueError("a node with one child")
        if len(root.kids) not in (2, 3):
            raise ValueError("tree has %d top level nodes. Only 2 and 3 are valid." % len(root.kids))       # TreeParser.java:164
        everything = frozenset(self.leaves)

        def length(nd):                                    # BasicTree.java:286, :497-507
            return float(nd.length) if use_lengths and nd.length is not None else 0.0

        # node indices of the round-tripped text: children reordered, leaves in text order, inner nodes by ')'
        jleaf, jinner = [], []

        def walk(nd):
            if nd.is_leaf():
                jleaf.append(nd)
                return
            for k in [k for k in nd.kids if k.is_leaf()] + [k for k in nd.kids if not k.is_leaf()]:
                walk(k)
            jinner.append(nd)

        walk(root)
        self.branches, top = [], []
        for nd in jleaf + jinner:
            if nd is root:
                continue
            if any(nd is k for k in root.kids):            # TreeParser.java:85-100
                top.append(nd)
                continue
            below = frozenset(leaves_below(nd))            # nodeA = the child (:105-108)
            self.branches.append(Branch(below, everything - below, length(nd)))
        if len(top) == 2:                                  # :138-151
            a, b = frozenset(leaves_below(top[0])), frozenset(leaves_below(top[1]))
            self.branches.append(Branch(a, b, length(top[0]) + length(top[1])))
        else:                                              # :152-162
            for nd in top:
                below = frozenset(leaves_below(nd))
                self.branches.append(Branch(below, everything - below, length(nd)))
        self._clades = self._map = None

    @classmethod
    def from_branches(cls, leaves, branches):
        """a tree given by its branch list [(side0, side1, length)]: for cases that no text produces (a repeated split)"""
        t = object.__new__(cls)
        t.root, t.leaves = None, list(leaves)
        t.branches = [Branch(a, b, float(l)) for a, b, l in branches]
        t._clades = t._map = None
        return t

    # Tree.getCladeSet, Tree.java:505-524: BOTH leaf sets of every branch
    def clade_set(self):
        if self._clades is None:
            r = set()
            for b in self.branches:
                r.add(b.sides[0])
                r.add(b.sides[1])
            self._clades = r
        return self._clades

    # tree2SetsToBranches, TreeComparison.java:629-637: HashMap.put of both leaf sets of every branch, in branch order
    def sets_to_branches(self):
        if self._map is None:
            m = {}
            for i, b in enumerate(self.branches):
                m[b.sides[0]] = i
                m[b.sides[1]] = i
            self._map = m
        return self._map

    def max_length(self):                                  # StatisticsUtilities.getMaximum :194-205
        r = -math.inf
        for b in self.branches:
            if b.length == b.length:
                r = max(r, b.length)
        return r


def robinson_foulds_legacy(t1, t2):
    """Tree.getRobinsonFouldsDistance, Tree.java:589-603"""
    a, b = t1.clade_set(), t2.clade_set()
    return (len(a | b) - len(a & b)) // 4


# ---- AdvancedTree.getRobinsonFouldsDistance, AdvancedTree.java:1460-1483 ----
def bipartition(side_bits, size):
    """Bipartition(ExtendedBitSet, int), Bipartition.java:41-64 -> (smallerSide, largerSide) as ints"""
    comp = ~side_bits & ((1 << size) - 1)
    a, b = bin(side_bits).count("1"), bin(comp).count("1")
    if a < b:
        return (side_bits, comp)
    if a > b:
        return (comp, side_bits)
    first = lambda x: (x & -x).bit_length() - 1 if x else -1        # nextSetBit(0)
    return (side_bits, comp) if first(side_bits) < first(comp) else (comp, side_bits)


_DESCENDANTS = {}      # text -> (leaf count, descendant leaves of every node): parsed once per text, not once per pair


def advanced_bipartitions(text, taxa):
    """AdvancedTree.getBipartitions(taxonNames), AdvancedTree.java:1291-1333, on the tree as its text roots it: every node with
    more than 1 and fewer than n - 1 descendant leaves (:1312; TreeComparison.getTreeBipartitions :354 is the same test).
    Bipartition.equals compares both sides (Bipartition.java:292-303): tuples compare the same way"""
    if text not in _DESCENDANTS:
        root = parse_newick(text)
        _DESCENDANTS[text] = (len(leaves_below(root)), [leaves_below(nd) for nd in all_nodes(root)])
    nleaves, descendants = _DESCENDANTS[text]
    index = {t: i for i, t in enumerate(taxa)}
    out = []
    for d in descendants:
        if 1 < len(d) < nleaves - 1:
            bits = 0
            for x in d:
                if x in index:
                    bits |= 1 << index[x]
            out.append(bipartition(bits, len(taxa)))
    return out


def robinson_foulds_bipartition(text1, text2):
    advanced_bipartitions(text1, [])
    taxa = _DESCENDANTS[text1][1][0]                       # this.getLeafLabels(): the root's descendants
    a, b = set(advanced_bipartitions(text1, taxa)), set(advanced_bipartitions(text2, taxa))
    return (len(a | b) - len(a & b)) // 2


# ---- the two distances ----
def _div(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def _finish(r, ss1, ss2):
    with np.errstate(all="ignore"):
        return float(np.sqrt(np.float64(r)) / np.sqrt(np.float64(ss1 + ss2)))


def branch_distance_sums(t1, t2):
    """getBranchDistance, TreeComparison.java:607-747 -> (r, sumOfSquaresTree1, sumOfSquaresTree2)"""
    max1, max2 = t1.max_length(), t2.max_length()                         # :641, :647
    len1 = [_div(b.length, max1) for b in t1.branches]                    # :643-645
    len2 = [_div(b.length, max2) for b in t2.branches]                    # :649-651
    to2 = t2.sets_to_branches()
    r = ss1 = ss2 = 0.0
    checked = set()
    for i, b in enumerate(t1.branches):                                   # :657-697, tree 1's order
        c = to2.get(b.sides[1])                                           # :662
        counterpart = _div(t2.branches[c].length, max2) if c is not None else 0.0      # :664
        bl = len1[i]
        ss1 += bl * bl                                                    # :692
        d = bl - counterpart
        r += d * d                                                        # :694
        checked.add(c)                                                    # :696
    for i in range(len(t2.branches)):                                     # :737-743, tree 2's order
        bl = len2[i]
        ss2 += bl * bl
        if i not in checked:
            r += bl * bl
    return r, ss1, ss2


def discrepant_distance_sums(t1, t2):
    """getDiscrepantBranchDistance, TreeComparison.java:756-810: raw lengths, unmatched branches only"""
    to2 = t2.sets_to_branches()
    r = ss1 = ss2 = 0.0
    checked = set()
    for b in t1.branches:                                                 # :783-794
        bl = b.length
        ss1 += bl * bl
        c = to2.get(b.sides[0])
        if c is None:
            d = bl - 0.0
            r += d * d
        checked.add(c)
    for i, b in enumerate(t2.branches):                                   # :800-806
        bl = b.length
        ss2 += bl * bl
        if i not in checked:
            r += bl * bl
    return r, ss1, ss2


def branch_distance(t1, t2):
    return _finish(*branch_distance_sums(t1, t2))                         # :745


def discrepant_distance(t1, t2):
    return _finish(*discrepant_distance_sums(t1, t2))                     # :808


# ---- split records, as pml_debug_tree_splits lays them out ----
def split_int(side, index, n):
    """a leaf set as an int over the sorted names, normalised: the side with fewer leaves, on a tie the side holding taxon 0"""
    bits = 0
    for x in side:
        bits |= 1 << index[x]
    m = bin(bits).count("1")
    if 2 * m > n or (2 * m == n and not bits & 1):
        bits = ~bits & ((1 << n) - 1)
        m = n - m
    return bits, m <= 1


def ladder_splits(root):
    """the splits Tree::parse (host.cpp Builder::build) adds below the root when it resolves a node of m >= 3 children, taken in
    TEXT order, into a ladder: k0+k1, k0+k1+k2, ... k0+..+km-2.  They serve rf_splits (== pml_rf_distance) alone"""
    out = []
    nodes = list(all_nodes(root))[1:]
    for nd in nodes:
        if len(nd.kids) >= 3:
            acc = list(leaves_below(nd.kids[0]))
            for k in nd.kids[1:-1]:
                acc = acc + leaves_below(k)
                out.append(frozenset(acc))
    return out


def records(text, use_lengths=True):
    """[(split int, length, length / max, flags)] of one tree: its branches in branch order, then its ladder splits"""
    t = JTree(text, use_lengths)
    names = sorted(t.leaves)
    index = {x: i for i, x in enumerate(names)}
    n = len(names)
    mx = t.max_length()
    out = []
    for b in t.branches:
        s, triv = split_int(b.sides[0], index, n)
        out.append([s, b.length, _div(b.length, mx), REAL | (TRIVIAL if triv else 0)])
    for side in ladder_splits(t.root):
        s, triv = split_int(side, index, n)
        out.append([s, 0.0, 0.0, TRIVIAL if triv else 0])
    last = {}
    for i, r in enumerate(out):
        last[r[0]] = i
    for i in last.values():
        out[i][3] |= LAST
    return [tuple(r) for r in out]


def resolved_splits(text):
    """the non-trivial splits of the tree as Tree::parse resolves it"""
    return {r[0] for r in records(text, False) if not r[3] & TRIVIAL}


def rf_splits(text1, text2):
    a, b = resolved_splits(text1), resolved_splits(text2)
    return (len(a) + len(b) - 2 * len(a & b)) // 2


# ---- the pair schedule ----
class TreeSet:
    """the trees of a call, parsed once"""

    def __init__(self, texts, use_lengths=True):
        self.texts = list(texts)
        self.trees = [JTree(x, use_lengths) for x in texts]
        first = sorted(self.trees[0].leaves)
        for t in self.trees:
            if sorted(t.leaves) != first:
                raise ValueError("unequal leaf sets")
        self.resolved = [resolved_splits(x) for x in texts]

    def pair(self, i, j):
        """tree 1 = i -> (rf_legacy, rf_bipartition, rf_splits, branch_dist, discrepant_dist)"""
        a, b = self.trees[i], self.trees[j]
        ra, rb = self.resolved[i], self.resolved[j]
        return (robinson_foulds_legacy(a, b), robinson_foulds_bipartition(self.texts[i], self.texts[j]),
                (len(ra) + len(rb) - 2 * len(ra & rb)) // 2, branch_distance(a, b), discrepant_distance(a, b))

    def compare_all(self, window=0):
        """compareAllvsAll(TreeI[]), TreeComparison.java:267-288: pair (i, j) for i < j only, tree 1 = i, [j][i] a copy; the
        diagonal: 0 and the formula's own value; window w > 0: only |i - j| <= w (compareSlidingWindow :241-265 and
        rollingComparison :457-466 are such bands), the rest -1 / NaN"""
        T = len(self.trees)
        rf = np.full((3, T, T), -1, dtype=np.int32)
        dist = np.full((2, T, T), np.nan)
        for i in range(T):
            for j in range(i, T):
                if window > 0 and j - i > window:
                    continue
                p = self.pair(i, j)
                for k in range(3):
                    rf[k, i, j] = rf[k, j, i] = 0 if i == j else p[k]
                for k in range(2):
                    dist[k, i, j] = dist[k, j, i] = p[3 + k]
        return {"rf_legacy": rf[0], "rf_bipartition": rf[1], "rf_splits": rf[2], "branch_dist": dist[0], "discrepant_dist": dist[1]}


def compare_one(standard, texts, use_lengths=True):
    """calculateTreeDistances, TreeComparison.java:557-565: the standard tree is tree 1"""
    s = TreeSet([standard] + list(texts), use_lengths)
    rows = [s.pair(0, j) for j in range(1, len(s.trees))]
    return {"rf_legacy": np.array([r[0] for r in rows], dtype=np.int32), "rf_bipartition": np.array([r[1] for r in rows], dtype=np.int32),
            "rf_splits": np.array([r[2] for r in rows], dtype=np.int32), "branch_dist": np.array([r[3] for r in rows]),
            "discrepant_dist": np.array([r[4] for r in rows])}


# ---- the closed form the device path uses ----
def pair_counts(t1, t2):
    """(shared, shared non-trivial, distinct and distinct non-trivial of t1, the same of t2) over the trees' distinct splits"""
    def splits(t):
        n = len(t.leaves)
        every = {frozenset(b.sides) for b in t.branches}
        return every, {s for s in every if min(len(x) for x in s) > 1 and n > 0}
    a, an = splits(t1)
    b, bn = splits(t2)
    return len(a & b), len(an & bn), len(a), len(an), len(b), len(bn)


def rf_closed_form(distinct_a, distinct_b, shared):
    """A tree's clade set holds the two leaf sets of each of its d distinct splits: 2 d sets (the two sides of a split differ
    and no set belongs to two splits).  Two trees over the same leaves share 2 s sets.  |union| - |intersection| =
    (2 dA + 2 dB - 2 s) - 2 s = 2 (dA + dB - 2 s), and the Java divides by 4 in ints: (dA + dB - 2 s) // 2.  With Bipartitions
    (one object per split) the difference is dA + dB - 2 s and the Java divides by 2: the same expression"""
    return (distinct_a + distinct_b - 2 * shared) // 2


# ---- drawing tree sets: one random tree perturbed by random NNIs and SPRs ----
def random_tree(rng, names):
    """a random unrooted binary tree (top level of three) as nested lists of names"""
    parts = list(names)
    while len(parts) > 3:
        i, j = sorted(rng.choice(len(parts), 2, replace=False))
        a, b = parts[i], parts[j]
        parts = [x for k, x in enumerate(parts) if k not in (i, j)] + [[a, b]]
    return parts


def _inner_paths(t, path=()):
    for i, k in enumerate(t):
        if isinstance(k, list):
            yield path + (i,)
            yield from _inner_paths(k, path + (i,))


def _all_paths(t, path=()):
    for i, k in enumerate(t):
        yield path + (i,)
        if isinstance(k, list):
            yield from _all_paths(k, path + (i,))


def _get(t, path):
    for i in path:
        t = t[i]
    return t


def _copy(t):
    return [_copy(k) if isinstance(k, list) else k for k in t]


def nni(rng, t):
    """swap a child of a random inner node with a sibling of that node"""
    t = _copy(t)
    paths = list(_inner_paths(t))
    if not paths:
        return t
    p = paths[rng.integers(len(paths))]
    parent, node = _get(t, p[:-1]), _get(t, p)
    sib = [i for i in range(len(parent)) if i != p[-1]]
    s = sib[rng.integers(len(sib))]
    c = rng.integers(len(node))
    parent[s], node[c] = node[c], parent[s]
    return t


def spr(rng, t):
    """cut a random subtree off and put it back on a random edge of the rest"""
    for _ in range(50):
        u = _copy(t)
        paths = [p for p in _all_paths(u)]
        p = paths[rng.integers(len(paths))]
        parent = _get(u, p[:-1])
        if len(p) == 1 and len(parent) <= 3:
            continue                                       # keep a top level of three
        sub = parent.pop(p[-1])
        if len(parent) == 1 and len(p) > 1:                # collapse the unary node
            grand = _get(u, p[:-2])
            grand[p[-2]] = parent[0]
        targets = list(_all_paths(u))
        q = targets[rng.integers(len(targets))]
        host = _get(u, q[:-1])
        host[q[-1]] = [host[q[-1]], sub]
        if len(u) == 3:
            return u
    return _copy(t)


def to_newick(t, rng=None, lengths=True, digits=6, zero=False, drop=0.0):
    def sub(x):
        s = "(" + ",".join(sub(k) for k in x) + ")" if isinstance(x, list) else x
        if lengths and not (drop and rng.random() < drop):
            s += ":" + ("0.0" if zero else repr(round(float(rng.uniform(0.001, 1.0)), digits)))
        return s
    return "(" + ",".join(sub(k) for k in t) + ");"


def _splits_of(t, names):
    every = frozenset(names)
    out = set()

    def sub(x):
        if not isinstance(x, list):
            return frozenset([x])
        s = frozenset().union(*[sub(k) for k in x])
        if 1 < len(s) < len(every) - 1:
            out.add(frozenset([s, every - s]))
        return s
    for k in t:
        sub(k)
    return out


def collapse(rng, t):
    """a multifurcation: one random inner node below the top level is dissolved into its parent"""
    t = _copy(t)
    paths = [p for p in _inner_paths(t) if len(p) >= 2]        # never into the top level: four top-level nodes are no tree
    if not paths:
        return t
    p = paths[rng.integers(len(paths))]
    parent = _get(t, p[:-1])
    node = parent.pop(p[-1])
    for k in reversed(node):
        parent.insert(p[-1], k)
    return t


def draw_set(n, T, seed, moves=None):
    """T trees of n taxa.  Tree 0 is a random tree with lengths; in this order, as far as T reaches:
      1  tree 0's text again                                       (two identical trees)
      2  a tree that shares no non-trivial split with tree 0, one inner node dissolved where n allows it, rooted at a bifurcating
         top level, every length 0.0            (nothing in common beyond the pendant branches; multifurcation; all lengths zero)
      3  tree 0's topology with other lengths                      (one topology, different lengths)
      4  a perturbed tree with a multifurcation and some lengths missing
      5  a perturbed tree without any length
      6+ tree 0 after k random moves (NNI or SPR), k growing with the index, so that pairs share anything from all splits to few
    The parser admits no repeated split (a node with one child is refused), so no set holds one."""
    rng = np.random.default_rng(seed)
    names = ["t%03d" % i for i in range(n)]
    base = random_tree(rng, names)
    texts = [to_newick(base, rng)]
    for k in range(1, T):
        if k == 1:
            texts.append(texts[0])
        elif k == 2:
            s0 = _splits_of(base, names)
            other = None
            for _ in range(2000):
                perm = [names[i] for i in rng.permutation(n)]
                cat = perm[0]
                for x in perm[1:-2]:
                    cat = [cat, x]
                cand = [cat, perm[-2], perm[-1]] if n > 3 else perm
                if not (_splits_of(cand, names) & s0):
                    other = cand
                    break
            assert other is not None, "no tree without a shared split found"
            if n >= 6:
                other = collapse(rng, other)
            rooted = [[other[0], other[1]], other[2]] if n > 4 else other      # bifurcating top; keeps the splits (n > 4: a new one would be trivial or old)
            texts.append(to_newick(rooted if _splits_of(rooted, names) == _splits_of(other, names) else other, rng, zero=True))
        elif k == 3:
            texts.append(to_newick(base, rng))
        elif k == 4:
            t = collapse(rng, spr(rng, base)) if n >= 6 else spr(rng, base)
            texts.append(to_newick(t, rng, drop=0.3))
        elif k == 5:
            texts.append(to_newick(nni(rng, base), lengths=False))
        else:
            t = base
            for _ in range(int(moves) if moves else 1 + (k * 7) % max(2, n)):
                t = nni(rng, t) if rng.random() < 0.5 else spr(rng, t)
            texts.append(to_newick(t, rng))
    return texts
