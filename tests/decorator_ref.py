"""TreeSupportDecorator.addSupportValues restated in Python from the Java, for the support-rule tests.

Read from the reference line by line (package edu.vt.vbi.ci.pepr.tree):

* TreeSupportDecorator.java:86-163  addSupportValues(main, supports)
    :90-98    every string becomes an AdvancedTree and is passed through unroot()
    :102-103  taxa = the MAIN tree's leaf labels, Arrays.sort (UTF-16 code units: plain string order for ASCII names)
    :108-122  main node i -> Bipartition(bits of its descendant leaves found in taxa, taxa.length)
    :126-142  EVERY node j of EVERY support tree -> Bipartition(bits of its descendant leaves found in taxa -- a leaf that
              Arrays.binarySearch does not find sets nothing, :134-137 --, taxa.length), added to ONE BipartitionSet
    :146-148  a main node's count = BipartitionSet.getCount(its bipartition)
* BipartitionSet.java:155-164, 334-341  add() increments a HashMap<Bipartition, Integer>: a multiset, a tree may add the same
              bipartition more than once
* Bipartition.java:41-64   the complement is taken over `size` (= the MAIN taxon count); smaller side by cardinality; equal
              cardinalities: the side whose nextSetBit(0) is lower, i.e. the side holding the lowest index
              :281-303  equality / hash = the two sides
* BasicTree.java:388-408, 597-606  a tree is "rooted" when its top-level node has exactly two children
              :669-717  unroot(): rootChildren[0] becomes the parent of rootChildren[1] (the other way round when
              rootChildren[0] has fewer than two children); the old root stays in the node arrays without children
* AdvancedTree.java:560-598  getDescendantLeaves(node): the labels of the childless nodes below it; an index past the leaf
              label array (the childless old root) contributes no label -> an empty set

The engine prints its labels where pml_support_tree prints them, so the tests compare per main split, not per string.
`restricted_counts` is the restatement of the rooting-independent rule 2 of include/peprml.h.
"""
import re


class Node:
    def __init__(self):
        self.kids, self.name, self.label, self.was_leaf = [], None, None, False


def parse(newick):
    """rooted tree exactly as the text nests it; inner labels (supports) kept, lengths dropped"""
    s = newick.strip().rstrip(";")
    pos = 0

    def node():
        nonlocal pos
        v = Node()
        if s[pos] == "(":
            pos += 1
            while True:
                v.kids.append(node())
                if s[pos] == ",":
                    pos += 1
                    continue
                assert s[pos] == ")", (s, pos)
                pos += 1
                break
        m = re.match(r"([^,():;\[\]]*)(:[-+0-9.eE]+)?", s[pos:])
        pos += len(m.group(0))
        if v.kids:
            v.label = m.group(1) or None
        else:
            v.name, v.was_leaf = m.group(1), True
        return v
    root = node()
    assert pos == len(s), (s, pos)
    return root


def nodes_of(root):
    out, stack = [], [root]
    while stack:
        v = stack.pop()
        out.append(v)
        stack.extend(v.kids)
    return out


def unroot(root):
    """BasicTree.unroot(): returns every node of the node arrays (the childless old root included)"""
    every = nodes_of(root)
    if len(root.kids) == 2:                                       # isRooted()
        new_parent, new_child = root.kids
        if len(new_parent.kids) < 2:                              # :693-696
            new_parent, new_child = new_child, new_parent
        new_parent.kids = new_parent.kids + [new_child]           # :698-703
        root.kids = []                                            # :706
    return every


def descendant_leaves(v):
    """AdvancedTree.getDescendantLeaves: labels of the childless nodes below v that index the leaf-label array"""
    if not v.kids:
        return [v.name] if v.was_leaf else []
    out = []
    for c in v.kids:
        out += descendant_leaves(c)
    return out


def bipartition(indices, size):
    """Bipartition(ExtendedBitSet, size) -> its smaller side, a frozenset of taxon indices"""
    bipart = frozenset(indices)
    complement = frozenset(range(size)) - bipart
    if len(bipart) != len(complement):
        return bipart if len(bipart) < len(complement) else complement
    first = lambda b: min(b) if b else -1                         # nextSetBit(0)
    return bipart if first(bipart) < first(complement) else complement


def _main_taxa(main_newick):
    return sorted(v.name for v in nodes_of(parse(main_newick)) if v.was_leaf)


def _bits(v, taxa):
    index = {t: i for i, t in enumerate(taxa)}
    return [index[x] for x in descendant_leaves(v) if x in index]


def decorator_counts(main_newick, support_newicks):
    """{smaller side (frozenset of taxon NAMES): count} for every main node whose smaller side holds >= 2 taxa"""
    taxa = _main_taxa(main_newick)
    n = len(taxa)
    multiset = {}
    for s in support_newicks:
        for v in unroot(parse(s)):
            b = bipartition(_bits(v, taxa), n)
            multiset[b] = multiset.get(b, 0) + 1
    out = {}
    for v in unroot(parse(main_newick)):
        b = bipartition(_bits(v, taxa), n)
        if len(b) >= 2:
            out[frozenset(taxa[i] for i in b)] = multiset.get(b, 0)
    return out


def restricted_counts(main_newick, support_newicks):
    """rule 2: a tree over S supports A|B when |A & S| >= 2, |B & S| >= 2 and one of its edges cuts S into A & S | B & S"""
    taxa = _main_taxa(main_newick)
    n, out = len(taxa), {}
    trees = []
    for s in support_newicks:
        root = parse(s)
        S = frozenset(_bits(root, taxa))
        trees.append((S, {frozenset(_bits(v, taxa)) for v in nodes_of(root)}))
    for v in nodes_of(parse(main_newick)):
        A = frozenset(_bits(v, taxa))
        if len(bipartition(A, n)) < 2:
            continue
        cnt = 0
        for S, below in trees:
            a, b = A & S, S - A
            cnt += len(a) >= 2 and len(b) >= 2 and (a in below or b in below)
        out[frozenset(taxa[i] for i in bipartition(A, n))] = cnt
    return out


def labelled_counts(labelled_newick):
    """the same table read back from an engine string: {smaller side: integer inner label}"""
    root = parse(labelled_newick)
    taxa = sorted(v.name for v in nodes_of(root) if v.was_leaf)
    out = {}
    for v in nodes_of(root):
        if v.kids and v.label is not None:
            b = bipartition(_bits(v, taxa), len(taxa))
            key = frozenset(taxa[i] for i in b)
            assert key not in out, "two labels for one split"
            out[key] = int(v.label)
    return out
