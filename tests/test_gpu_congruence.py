"""The congruence filter on the device (congruence.hip through pml_congruence_costs / pml_congruence_filter) against the Python
restatement tests/congruence_ref.py.  Everything is sets and integer sums, so every comparison is for equality."""
import os

import numpy as np
import pytest

from pepr_amd import engine, tree_builder
import congruence_ref as ref
from test_congruence_host import evolve, planted_genes, random_tree

pytestmark = pytest.mark.gpu
BYTES = list("ACDEFG" + "acdefg" + "X-?")


# ---- 1. extraction alone: the records k_colsplits wrote, per column, against the restatement ----
def _extraction_cases():
    out = []
    for ntax in (2, 4, 31, 32, 33, 63, 64, 65, 129, 257, 512):          # every W, both sides of every word boundary
        for ncols in ((1, 63, 64, 65, 257) if ntax in (64, 65, 512) else (1, 65, 257) if ntax in (2, 32, 33, 129, 257) else (63, 64)):
            out.append((ntax, ncols))
    return out


@pytest.mark.parametrize("ntax,ncols", _extraction_cases())
def test_column_splits(gpu_ctx, ntax, ncols):
    rng = np.random.default_rng(100000 * ntax + ncols)
    union = ["n%04d" % i for i in range(ntax)]
    cols = rng.choice(BYTES, (ncols, ntax))
    half = np.array(["A"] * (ntax // 2) + ["C"] * (ntax - ntax // 2))
    forced = {0: half, 5: half[::-1], 11: np.array(["-", "?"] * ntax)[:ntax], 17: rng.permutation(half), 40: np.array(["?"] * ntax),
              64: half, 70: np.array(["-"] * ntax), 200: half[::-1], 256: rng.permutation(half)}
    for c, v in forced.items():                                    # two classes (a tie at even ntax, both orientations) and all-gap columns
        if c < ncols:
            cols[c] = v
    # the gene has all taxa, or (odd ncols) lacks one from the middle; its rows come in shuffled order
    have = [t for t in range(ntax) if not (ncols % 2 and ntax >= 4 and t == ntax // 2)]
    order = rng.permutation(have)
    gene = ([union[t] for t in order], ["".join(cols[:, t]) for t in order])
    want = ref.gene_column_splits(gene, union)
    got = gpu_ctx.debug_column_splits(gene, union)
    assert [c for c, _ in got] == sorted(c for c, _ in got)        # records in column order
    per_col = [[] for _ in range(ncols)]
    for c, s in got:
        per_col[c].append(s)
    for c in range(ncols):
        assert len(per_col[c]) == len(set(per_col[c])), c          # the duplicate of two covering classes was dropped
        assert set(per_col[c]) == (want[c] or set()), (c, "".join(cols[c]))
    if len(have) == ntax:
        assert len(per_col[0]) == 1                                # the forced two-class column is one split
        if ntax % 2 == 0 and ncols > 5:
            assert per_col[0] == per_col[5] == [(1 << (ntax // 2)) - 1]      # the tie keeps the side with taxon 0, whichever class that is


# ---- 2. the whole call ----
def _subset_genes(seed, ntax, ngenes, ncols):
    """genes evolved down one random tree (one gene down another), over different taxon subsets: most lack one to three
    taxa, the last covers only 3"""
    rng = np.random.default_rng(seed)
    names = ["tx%03d" % i for i in range(ntax)]
    main, other = random_tree(rng, ntax), random_tree(rng, ntax)
    genes = []
    for g in range(ngenes):
        rows = evolve(rng, *(other if g == 1 else main), ntax, ncols + g)
        lack = set(rng.choice(ntax, int(rng.integers(0, 4)), replace=False).tolist()) if g else set()
        keep = [t for t in range(ntax) if t not in lack] if g < ngenes - 1 else sorted(rng.choice(ntax, 3, replace=False).tolist())
        keep = [keep[i] for i in rng.permutation(len(keep))]
        genes.append(([names[t] for t in keep], [rows[t] for t in keep]))
    return genes


WHOLE = {12: (11, 20, 60), 33: (12, 12, 40), 65: (13, 8, 30), 129: (14, 6, 30)}      # ntax: seed, genes, columns
_cache = {}


def _whole(ntax):
    if ntax not in _cache:
        genes = _subset_genes(*((WHOLE[ntax][0], ntax) + WHOLE[ntax][1:]))
        _cache[ntax] = (genes, ref.congruence_filter(genes, 0.1))
    return _cache[ntax]


def _same_costs(got, want):
    assert got["names"] == want["names"] and got["n"] == want["n"]
    assert got["cutoff"] == want["cutoff"]
    assert len(got["kept_splits"]) == len(want["kept"]) and set(got["kept_splits"]) == ref.kept_splits(want)
    for key in ("cost_sum", "mean_cost", "nsplits"):
        assert got[key] == want[key], key


@pytest.mark.parametrize("mask", [None, 0xF, 0], ids=["ones", "0xF", "zero"])
@pytest.mark.parametrize("ntax", sorted(WHOLE))
def test_whole_call(gpu_ctx, ntax, mask):
    genes, want = _whole(ntax)
    assert len({frozenset(g[0]) for g in genes}) > 3 and min(len(g[0]) for g in genes) == 3
    assert any(want["cost_sum"]) and len(want["names"]) == ntax
    if ntax == 12:
        assert want["cutoff"] > 0 and len(want["kept"]) < len(want["counts"])      # the top-N rule cut something off
    if ntax == 129:
        assert len(want["kept"]) == len(want["counts"]) > 2 * engine.congruence_ktile()   # K is every counted split: several LDS tiles
    got = gpu_ctx.congruence_costs(genes, hash_mask=mask)
    _same_costs(got, want)
    ints = [sum(int(x) << (64 * i) for i, x in enumerate(row)) for row in got["kept_words"]]
    assert ints == sorted(ints)                                     # K ascending as n-bit integers
    if mask is None:
        f = gpu_ctx.congruence_filter(genes, 0.1)
        _same_costs(f, want)
        assert (f["keep"], f["idx"], f["max_cost"]) == (want["keep"], want["idx"], want["max_cost"])


def test_kept_set_larger_than_the_lds_tile(gpu_ctx):
    """|K| at least twice k_splitcost's tile: one two-class column per random split, fewer columns than 4 n, so K is all of them"""
    tile = engine.congruence_ktile()
    total = 2 * tile + 48
    n = total // 4 + 10
    assert n <= 512 and total < 4 * n
    rng = np.random.default_rng(tile)
    names = ["s%03d" % i for i in range(n)]
    cols = []
    for _ in range(total):
        inside = set(rng.choice(n, int(rng.integers(2, n // 2)), replace=False).tolist())
        cols.append("".join("A" if t in inside else "C" for t in range(n)))
    per = total // 4
    genes = [(names, ["".join(c[t] for c in cols[g * per:(g + 1) * per]) for t in range(n)]) for g in range(4)]
    want = ref.congruence_costs(genes)
    assert len(want["kept"]) >= 2 * tile and any(want["cost_sum"])
    _same_costs(gpu_ctx.congruence_costs(genes), want)


def test_two_runs_give_identical_bytes(gpu_ctx):
    genes, _ = _whole(33)
    for mask in (None, 0xF):
        a, b = gpu_ctx.congruence_costs(genes, hash_mask=mask), gpu_ctx.congruence_costs(genes, hash_mask=mask)
        assert a["kept_words"].tobytes() == b["kept_words"].tobytes()
        assert {k: v for k, v in a.items() if k != "kept_words"} == {k: v for k, v in b.items() if k != "kept_words"}


def test_planted_gene_is_dropped(gpu_ctx):
    genes = planted_genes()
    want = ref.congruence_filter(genes, 0.1)
    got = gpu_ctx.congruence_filter(genes, 0.1)
    assert got["keep"] == want["keep"] and [g for g, k in enumerate(got["keep"]) if not k] == [3, 19]
    assert got["mean_cost"] == want["mean_cost"]
    kept = tree_builder.filterForCongruence(genes, 0.1, ctx=gpu_ctx)
    assert kept == [g for i, g in enumerate(genes) if i not in (3, 19)]


def test_refusals(gpu_ctx, monkeypatch):
    ok = (["a", "b", "c"], ["AC", "AC", "CA"])
    with pytest.raises(engine.PmlError) as e:                       # a gene without columns
        gpu_ctx.congruence_costs([ok, (["a", "b"], ["", ""])])
    assert e.value.code == -2 and "gene 1" in str(e.value)
    with pytest.raises(engine.PmlError) as e:                       # 513 taxa
        gpu_ctx.congruence_costs([(["u%03d" % i for i in range(513)], ["A"] * 513)])
    assert e.value.code == engine.EINVAL and "513" in str(e.value)
    for p in (0, -1, float("nan")):
        with pytest.raises(engine.PmlError) as e:
            gpu_ctx.congruence_filter([ok], p)
        assert e.value.code == engine.EINVAL
    rng = np.random.default_rng(1)
    big = (["b%02d" % i for i in range(64)], ["".join(r) for r in rng.choice(list("ACDE"), (64, 20000))])      # 1.28 MB of bytes alone
    monkeypatch.setenv("PML_HBM_BUDGET_MB", "1")
    with pytest.raises(engine.PmlError) as e:
        gpu_ctx.congruence_costs([big])
    assert e.value.code == -4 and "MiB" in str(e.value)
    monkeypatch.delenv("PML_HBM_BUDGET_MB")
    r = gpu_ctx.congruence_costs([ok])                              # the same context goes on working
    assert r["n"] == 3 and r["cost_sum"] == [0]


def test_tree_step_tool(gpu_ctx, tmp_path, monkeypatch, capsys):
    monkeypatch.syspath_prepend(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import pepr_tree_step
    genes = planted_genes()
    d = tmp_path / "alignments"
    d.mkdir()
    for i, (names, rows) in enumerate(genes):
        (d / ("fam%02d.fasta" % i)).write_text("".join(">%s\n%s\n" % (n, r) for n, r in zip(names, rows)))
    want = ref.congruence_filter(genes, 0.1)
    run = str(tmp_path / "filtered")
    pepr_tree_step.main(["-run_name", run, "-alignment_dir", str(d), "-support_reps", "4", "-seed", "3", "--full-tree-method", "nj",
                         "-congruence_filter", "-trim_percent", "0.1"])
    out = capsys.readouterr().out
    lines = open(run + ".congruence.tsv").read().splitlines()
    assert lines[0].split("\t") == ["file", "columns", "cost_sum", "mean_cost", "kept"]
    assert [l.split("\t") for l in lines[1:]] == [["fam%02d.fasta" % i, "60", str(want["cost_sum"][i]), str(want["mean_cost"][i]), str(int(want["keep"][i]))]
                                                  for i in range(20)]
    assert "discarding set fam03.fasta cost: %d" % want["mean_cost"][3] in out and "discarding set fam19.fasta" in out
    assert "Discarded: 2\tKept: 18" in out
    kept = [g for g, k in zip(genes, want["keep"]) if k]
    trees = gpu_ctx.nj_jackknife(kept, reps=4, seed=3, support_rule=engine.SUPPORT_DECORATOR)
    assert open(run + ".nwk").read() == trees["newick"] + "\n"                 # the trees are built on the kept genes only
    assert open(run + ".sup").read() == "\n".join(trees["support_trees"]) + "\n"
    # the double-dash spelling, and a run without the flag: what the tool wrote before the flags existed
    run2 = str(tmp_path / "dashes")
    pepr_tree_step.main(["-run_name", run2, "-alignment_dir", str(d), "-support_reps", "4", "-seed", "3", "--full-tree-method", "nj", "--congruence-filter"])
    assert open(run2 + ".congruence.tsv").read() == open(run + ".congruence.tsv").read() and open(run2 + ".nwk").read() == open(run + ".nwk").read()
    capsys.readouterr()
    run3 = str(tmp_path / "plain")
    pepr_tree_step.main(["-run_name", run3, "-alignment_dir", str(d), "-support_reps", "4", "-seed", "3", "--full-tree-method", "nj"])
    out = capsys.readouterr().out
    full = gpu_ctx.nj_jackknife(genes, reps=4, seed=3, support_rule=engine.SUPPORT_DECORATOR)
    assert open(run3 + ".nwk").read() == full["newick"] + "\n" and open(run3 + ".sup").read() == "\n".join(full["support_trees"]) + "\n"
    assert not os.path.exists(run3 + ".congruence.tsv") and "Discarded" not in out and len(out.splitlines()) == 1
    assert out.startswith(run3 + ": 20 genes, neighbor joining, 4 support trees")


def test_launch_accounting(gpu_ctx):
    genes, _ = _whole(33)
    before, sums_before = gpu_ctx.kernel_stats(), gpu_ctx.pairscore_sum_stats()["launches"]
    gpu_ctx.congruence_costs(genes)
    after = gpu_ctx.kernel_stats()
    cells = sum(len(g[0]) * len(g[1][0]) for g in genes)
    assert after["colsplit"]["launches"] - before["colsplit"]["launches"] == 2          # the count pass and the write pass
    assert after["colsplit"]["algo_bytes"] - before["colsplit"]["algo_bytes"] == 2 * cells
    assert after["splitcost"]["launches"] - before["splitcost"]["launches"] == 1
    assert after["splitcost"]["algo_bytes"] > before["splitcost"]["algo_bytes"]
    for name in after:
        if name not in ("colsplit", "splitcost"):
            assert after[name]["launches"] == before[name]["launches"], name
    assert gpu_ctx.pairscore_sum_stats()["launches"] == sums_before
