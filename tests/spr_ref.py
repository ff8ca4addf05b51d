"""SPR on unrooted binary trees, restated in Python from the definitions of include/peprml.h (pml_search2 and its two test
doors): the candidate regraft edges of a prune with their distances, the lazily regrafted tree, and Newick output.
Nothing here is shared with the engine; the tests compare the two."""
import itertools

from util import parse_newick


class UTree:
    """adj[v] = {neighbour: branch length}; leaves carry names in `name`."""

    def __init__(self, newick=None):
        self.adj, self.name = {}, {}
        if newick is None:
            return
        ids = itertools.count()

        def rec(nd):
            v = next(ids)
            self.adj[v] = {}
            if not nd[0]:
                self.name[v] = nd[1]
            for k in nd[0]:
                w = rec(k)
                self.adj[v][w] = self.adj[w][v] = k[2]
            return v
        root = rec(parse_newick(newick))
        if len(self.adj[root]) == 2:            # rooted binary top: suppress the root
            (a, la), (b, lb) = self.adj[root].items()
            del self.adj[root], self.adj[a][root], self.adj[b][root]
            self.adj[a][b] = self.adj[b][a] = la + lb

    def copy(self):
        t = UTree()
        t.adj = {v: dict(n) for v, n in self.adj.items()}
        t.name = dict(self.name)
        return t

    def leaves_behind(self, v, frm):
        """names of the leaves on v's side of edge (frm, v)"""
        out, st = [], [(v, frm)]
        while st:
            x, f = st.pop()
            if x in self.name:
                out.append(self.name[x])
            st.extend((w, x) for w in self.adj[x] if w != f)
        return frozenset(out)

    def inner(self):
        return [v for v in self.adj if v not in self.name]

    def prunes(self):
        """every (inner node p, neighbour s): the subtree behind s is cut off at p"""
        return [(p, s) for p in self.inner() for s in self.adj[p]]

    def node_behind(self, leaves):
        """(p, s) with leaves_behind(s, p) == leaves"""
        for p, s in self.prunes():
            if self.leaves_behind(s, p) == frozenset(leaves):
                return p, s
        raise KeyError(leaves)

    def newick(self, fmt="%.12g"):
        root = self.inner()[0]

        def rec(v, frm):
            kids = [w for w in self.adj[v] if w != frm]
            s = self.name[v] if v in self.name else "(" + ",".join(rec(w, v) for w in kids) + ")"
            return s + (":" + fmt % self.adj[v][frm] if frm is not None else "")
        return rec(root, None) + ";"


def candidates(t, p, s, rmin, rmax, allowed=None):
    """The regraft edges of the prune (p, s) from the definition: the edges of the pruned tree (p and the subtree behind s
    removed, p's other neighbours x, y joined) within rmin..rmax edges of the joined edge, the edge itself counted.
    -> {(far-side leaf set, distance): (g, h)}.  allowed(far_leaves) false: the edge and everything behind it drop out."""
    x, y = [w for w in t.adj[p] if w != s]
    out = {}
    frontier = [(x, w) for w in t.adj[x] if w != p] + [(y, w) for w in t.adj[y] if w != p]
    d = 1
    while frontier and d <= rmax:
        nxt = []
        for g, h in frontier:
            far = t.leaves_behind(h, g)
            if allowed is not None and not allowed(far):
                continue
            if d >= rmin:
                out[(far, d)] = (g, h)
            nxt.extend((h, w) for w in t.adj[h] if w != g)
        frontier, d = nxt, d + 1
    return out


def regraft_lazy(t, p, s, g, h):
    """the tree the lazy score belongs to: x-y joined with tx + ty, edge (g, h) halved around p, the pendant branch kept"""
    n = t.copy()
    x, y = [w for w in n.adj[p] if w != s]
    tx, ty = n.adj[p][x], n.adj[p][y]
    for w in (x, y):
        del n.adj[w][p], n.adj[p][w]
    n.adj[x][y] = n.adj[y][x] = tx + ty
    tgh = n.adj[g][h]
    del n.adj[g][h], n.adj[h][g]
    for w in (g, h):
        n.adj[w][p] = n.adj[p][w] = 0.5 * tgh
    return n


def split_set(t):
    """the non-trivial splits of the tree, each as the frozenset of its two sides"""
    out = set()
    allv = frozenset(t.name.values())
    for v in t.inner():
        for w in t.adj[v]:
            if w in t.name or w < v:
                continue
            a = t.leaves_behind(w, v)
            out.add(frozenset([a, allv - a]))
    return out


def spr_distance(before, after, rmax, rmin=1):
    """the distances rmin <= d <= rmax for which one SPR of `before` gives the topology of `after` (empty: none does)"""
    target, found = split_set(after), set()
    for p, s in before.prunes():
        if len(before.leaves_behind(s, p)) > len(before.name) - 3:
            continue
        for (far, d), (g, h) in candidates(before, p, s, rmin, rmax).items():
            if split_set(regraft_lazy(before, p, s, g, h)) == target:
                found.add(d)
    return found
