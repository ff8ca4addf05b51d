"""The three counting rules of pml_support_tree_rule / pml_jackknife2 (host only): rule 1 against the Python restatement of
TreeSupportDecorator.addSupportValues (tests/decorator_ref.py) and hand-derived fixtures, rule 2 against its own restatement,
rule 0 against pml_support_tree."""
import json
import os

import numpy as np
import pytest

import decorator_ref as dr
from pepr_amd import engine

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = json.load(open(os.path.join(HERE, "golden", "support_rule_cases.json")))["cases"]


def _keyed(table):
    return {frozenset(k.split(",")): v for k, v in table.items()}


def _canonical(table, main):
    """fixture keys name one side of a split as written; the engine and the references key by Bipartition's smaller side"""
    taxa = sorted(v.name for v in dr.nodes_of(dr.parse(main)) if v.was_leaf)
    out = {}
    for side, v in _keyed(table).items():
        b = dr.bipartition([taxa.index(t) for t in side], len(taxa))
        out[frozenset(taxa[i] for i in b)] = v
    return out


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_hand_derived_cases(case):
    main, sup = case["main"], case["supports"]
    for rule in (0, 1, 2):
        got = dr.labelled_counts(engine.support_tree_rule(main, sup, rule, 3))
        assert got == _canonical(case["expect"][str(rule)], main), (case["name"], rule)
    # the restatements agree with the paper too
    assert dr.decorator_counts(main, sup) == _canonical(case["expect"]["1"], main)
    assert dr.restricted_counts(main, sup) == _canonical(case["expect"]["2"], main)


def test_the_two_rootings_of_the_issue():
    main = "((a:1,b:1):1,(c:1,d:1):1,(e:1,f:1):1);"
    ab, cd, ef = frozenset("ab"), frozenset("cd"), frozenset("ef")
    one = dr.labelled_counts(engine.support_tree_rule(main, ["((a,b),(c,d),e);"], 1))
    two = dr.labelled_counts(engine.support_tree_rule(main, ["(a,b,((c,d),e));"], 1))
    assert one == {ab: 1, cd: 1, ef: 0} and two == {ab: 0, cd: 1, ef: 0}
    # rule 2 does not see the rooting
    assert engine.support_tree_rule(main, ["((a,b),(c,d),e);"], 2) == engine.support_tree_rule(main, ["(a,b,((c,d),e));"], 2)


# ---- random trees ----

def _random_unrooted(names, rng):
    """adjacency of a random binary unrooted tree (stepwise addition)"""
    adj = {names[0]: [names[1]], names[1]: [names[0]]}
    inner = 0
    for t in names[2:]:
        edges = [(u, v) for u in adj for v in adj[u] if str(u) < str(v)]
        u, v = edges[rng.integers(len(edges))]
        w = "#%d" % inner
        inner += 1
        adj[u].remove(v); adj[v].remove(u)
        adj[w] = [u, v, t]; adj[u].append(w); adj[v].append(w); adj[t] = [w]
    return adj


def _prune(adj, drop):
    adj = {u: list(vs) for u, vs in adj.items()}
    for t in drop:
        (w,) = adj.pop(t)
        adj[w].remove(t)
        if len(adj[w]) == 2:                                      # suppress the degree-2 node
            u, v = adj.pop(w)
            adj[u][adj[u].index(w)] = v; adj[v][adj[v].index(w)] = u
    return adj


def _write(adj, v, parent, rng, lengths):
    kids = [c for c in adj[v] if c != parent]
    rng.shuffle(kids)
    s = v if not kids else "(" + ",".join(_write(adj, c, v, rng, lengths) for c in kids) + ")"
    return s + (":%.3f" % rng.uniform(0.01, 1.0) if lengths and parent is not None else "")


def _newick(adj, rng, lengths=False):
    """the tree written from a random place: an inner node (trifurcating text) or the middle of an edge (two root children)"""
    inner = [u for u in adj if len(adj[u]) == 3]
    if rng.random() < 0.5 or not inner:
        edges = [(u, v) for u in adj for v in adj[u]]
        u, v = edges[rng.integers(len(edges))]
        return "(" + _write(adj, u, v, rng, lengths) + "," + _write(adj, v, u, rng, lengths) + ");"
    return _write(adj, inner[rng.integers(len(inner))], None, rng, lengths) + ";"


def _fuzz_case(rng):
    n = int(rng.integers(5, 13))
    names = ["t%02d" % i for i in rng.permutation(20)[:n]]
    main = _newick(_random_unrooted(names, rng), rng, lengths=True)
    sup = []
    for _ in range(int(rng.integers(1, 6))):
        tree = _random_unrooted(list(rng.permutation(names)), rng) if rng.random() < 0.5 else _random_unrooted(names, rng)
        k = min(int(rng.integers(0, 4)), n - 4)
        drop = list(rng.permutation(names)[:k])
        sup.append(_newick(_prune(tree, drop), rng, lengths=bool(rng.integers(2))))
    return main, sup


def test_fuzz_rules_1_and_2_equal_their_restatements():
    rng = np.random.default_rng(20240611)
    dropped = rooted2 = differ = 0
    for _ in range(400):
        main, sup = _fuzz_case(rng)
        one = dr.labelled_counts(engine.support_tree_rule(main, sup, 1, 3))
        two = dr.labelled_counts(engine.support_tree_rule(main, sup, 2, 3))
        assert one == dr.decorator_counts(main, sup), (main, sup)
        assert two == dr.restricted_counts(main, sup), (main, sup)
        dropped += any(s.count(",") < main.count(",") for s in sup)
        rooted2 += any(len(dr.parse(s).kids) == 2 for s in sup)
        differ += one != two
    assert dropped > 100 and rooted2 > 100 and differ > 20         # the generator reaches the cases the rules differ on


def test_equal_taxon_sets_all_rules_give_pml_support_tree():
    rng = np.random.default_rng(77)
    for _ in range(60):
        n = int(rng.integers(5, 13))
        names = ["s%d" % i for i in range(n)]
        main = _newick(_random_unrooted(names, rng), rng, lengths=True)
        sup = [_newick(_random_unrooted(names, rng) if rng.random() < 0.7 else _random_unrooted(names[::-1], rng), rng) for _ in range(4)]
        sup.append(main)
        want = engine.support_tree(main, sup, 4)
        for rule in (0, 1, 2):
            assert engine.support_tree_rule(main, sup, rule, 4) == want, (rule, main, sup)


def test_bad_arguments():
    main = "((a,b),(c,d),(e,f));"
    with pytest.raises(engine.PmlError):
        engine.support_tree_rule(main, [main], 3)
    with pytest.raises(engine.PmlError):
        engine.support_tree_rule(main, ["((a,b),(c,d)"], 1)
    with pytest.raises(engine.PmlError):
        engine.support_tree_rule(main, ["not a tree ("], 0)
    # rule 0 on a subset tree: counted as not supporting, where pml_support_tree refuses it
    assert dr.labelled_counts(engine.support_tree_rule(main, ["((a,b),(c,d),e);"], 0)) == {frozenset("ab"): 0, frozenset("cd"): 0, frozenset("ef"): 0}
