"""Gene sets for tests/test_gpu_genesteps.py, and a child process for its forced-budget test: run as a program it computes
gene_steps of budget_case() under whatever PML_HBM_BUDGET_MB its environment sets and prints the arrays' digests and the launch
counts as JSON."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LETTERS = "ACDEBZ-"                                # seven letters with seven different alignment codes


def random_trees(rng, names):
    """a random binary tree over `names` -> (unrooted text with a trifurcation at the top, the same tree rooted)"""
    nodes = list(names)
    while len(nodes) > 2:
        i, j = sorted(rng.choice(len(nodes), 2, replace=False))
        b = nodes.pop(j)
        a = nodes.pop(i)
        nodes.append("(%s,%s)" % (a, b))
    if not nodes[1].startswith("("):
        nodes.reverse()
    inner = nodes[1]                               # "(x,y)": its two children become top-level
    return "(%s,%s);" % (nodes[0], inner[1:-1]), "(%s,%s);" % (nodes[0], inner)


def distinct_columns(rng, ntax, count, avoid=()):
    """`count` columns over LETTERS, pairwise different (so `count` patterns), none of only '-', none in `avoid`"""
    seen, cols = set(avoid), []
    while len(cols) < count:
        c = "".join(rng.choice(list(LETTERS), ntax))
        if c in seen or set(c) <= {"-"}:
            continue
        seen.add(c)
        cols.append(c)
    return cols


def gene_of(names, cols, rng=None):
    """columns (strings over the gene's rows) -> (names, rows); with rng, some '-' become '?' or 'X': the same alignment code
    (so the same pattern) but other bytes"""
    rows = ["".join(c[r] for c in cols) for r in range(len(names))]
    if rng is not None:
        rows = ["".join(ch if ch != "-" else "-?X"[int(rng.integers(0, 3))] for ch in row) for row in rows]
        for k in range(len(cols)):                 # keep one plain letter or 'X' in every column: no column of only '-' and '?'
            if all(row[k] in "-?" for row in rows):
                rows[0] = rows[0][:k] + "X" + rows[0][k + 1:]
    return list(names), rows


def gene_set(ntax, seed, golden=None):
    """genes of 255, 256 and 257 patterns, one of 1000 columns over 100 patterns, one lacking two taxa; with `golden` (the five-taxon
    cases) their columns planted at both ends of two further genes, one of more than 256 patterns and one lacking E;
    planted = (gene, column in the gene, case)"""
    rng = np.random.default_rng(seed)
    names = ["t%02d" % i for i in range(ntax)] if golden is None else list(golden["taxa"])
    genes = [gene_of(names, distinct_columns(rng, ntax, n), rng) for n in (255, 256, 257)]
    base = distinct_columns(rng, ntax, 100)
    genes.append(gene_of(names, [base[int(i)] for i in rng.integers(0, 100, 1000)], rng))
    if ntax > 4:
        genes.append(gene_of(names[1:-1], distinct_columns(rng, ntax - 2, 60), rng))
    else:
        genes.append(gene_of(names[:3], distinct_columns(rng, 3, 60), rng))
    # few classes: columns of one or two letters over all rows, half of them with one '-' (two classes that cover all rows are
    # one bipartition, with a gap they are two)
    low = []
    for k in range(40):
        c = list(rng.choice(list("AC"), ntax)) if k % 4 else ["D"] * ntax
        if k % 2:
            c[int(rng.integers(0, ntax))] = "-"
        low.append("".join(c))
    genes.append(gene_of(names, low))
    planted = []
    if golden is not None:
        for absent in ([], ["E"]):
            own = [t for t in names if t not in absent]
            cases = [c for c in golden["cases"] if c["absent"] == absent and not c.get("refused")]
            gcols = ["".join(c["column"][names.index(t)] for t in own) for c in cases]
            filler = distinct_columns(rng, len(own), 300 if not absent else 40, avoid=gcols)
            h = len(gcols) // 2                    # the first half in front; behind the filler all of them, the second half as new patterns
            planted += [(len(genes), k, c) for k, c in enumerate(cases[:h])] + [(len(genes), h + len(filler) + k, c) for k, c in enumerate(cases)]
            genes.append(gene_of(own, gcols[:h] + filler + gcols))
    return names, genes, planted


def budget_case():
    rng = np.random.default_rng(65)
    names = ["t%02d" % i for i in range(65)]
    genes = [gene_of(names if k % 3 else names[2:], distinct_columns(rng, 65 if k % 3 else 63, 257 + k), rng) for k in range(12)]
    return names, genes, random_trees(rng, names)[0]


def digests(r):
    return {k: hashlib.sha256(np.ascontiguousarray(r[k]).tobytes()).hexdigest() for k in ("col_start", "steps", "min_steps", "gene_steps", "gene_beyond", "gene_ratio")}


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    from pepr_amd import engine
    ctx = engine.Context(0)
    _, genes, tree = budget_case()
    out = digests(ctx.gene_steps(genes, tree))
    out["stats"] = ctx.gene_steps_stats()
    out["budget"] = os.environ.get("PML_HBM_BUDGET_MB")
    ctx.close()
    print(json.dumps(out))
