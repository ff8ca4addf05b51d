"""Block trimming on the device (`-gblocks_trim`) against the restatement of the published rule (gblocks_ref.py), and the staged
call (pml_trim_pipeline) against the separate calls one after the other.  Every comparison is for equality."""
import json
import os
import re

import numpy as np
import pytest

from pepr_amd import engine, tree_builder
import congruence_ref as cref
import gblocks_ref as ref
import trim_ref
from test_congruence_host import evolve, random_tree

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "gblocks_cases.json")))
W = engine.gblocks_chunk()                                          # k_gbselect's chunk width
LDS_COLS = int(re.search(r"GB_LDS_COLS = (\d+)", open(os.path.join(ROOT, "pepr_amd", "csrc", "gblocks.hpp")).read()).group(1))
MODES = (ref.NONE, ref.HALF, ref.ALL)
OTHERS = np.frombuffer(b"CDEFGHIKLMNPQRSTVWY", dtype=np.uint8)


def small_params(n, gaps):
    """explicit parameters with b1 < b2 where n allows it (n >= 3), so that class 1 exists; the hand-worked cases' short thresholds"""
    b1 = n // 2 + 1
    return dict(GOLD["params"], b1=b1, b2=min(n, max(b1 + 1, 9 * n // 10)), gaps=gaps)


def column(n, top, gaps=0, second=0):
    """gaps '-', then top 'A', then second 'C', the rest cycling through 19 other residues"""
    top = max(0, min(top, n - gaps))
    second = max(0, min(second, n - gaps - top))
    rest = n - gaps - top - second
    return np.concatenate([np.full(gaps, ref.GAP, np.uint8), np.full(top, ord("A"), np.uint8), np.full(second, ord("C"), np.uint8),
                           np.resize(OTHERS[1:], rest) if rest else np.zeros(0, np.uint8)])


def class_column(ch, n, p):
    """a column of the class a hand-worked string names, at a threshold: top = n, b1, b1 - 1, or ceil(n / 2) gaps"""
    if ch == "g" or (ch == "0" and p["b1"] < 2):
        return column(n, n, gaps=(n + 1) // 2)
    return column(n, {"2": n, "1": p["b1"], "0": p["b1"] - 1}[ch])


def special_columns(n, p):
    """top at b1 - 1, b1, b2 - 1, b2; exactly n / 2 gaps; a tie of n / 2 (no majority); a majority of exactly b1 that alternates with
    the runner-up row by row"""
    cols = [column(n, t) for t in (p["b1"] - 1, p["b1"], p["b2"] - 1, p["b2"])]
    cols.append(column(n, n, gaps=n // 2))
    cols.append(column(n, n // 2, second=n // 2))
    k = n - p["b1"]
    cols.append(np.array([ord("A"), ord("C")] * k + [ord("A")] * (n - 2 * k), dtype=np.uint8))
    return cols


# the runs that must lie across a 64-column boundary and across a chunk boundary: (class string, index of the first column behind
# the boundary): a class-0 run of b3, one of b3 + 1, a block of b0, a gap position with class-0 neighbours
PIECES = (("22220002222", 5), ("222200002222", 6), ("000021120000", 6), ("222210g012222", 6))


def flags_gene(n, L, variant, gaps):
    """-> (gene, params, [(boundary, piece index, first column)])"""
    rng = np.random.default_rng(100000 * variant + 1000 * n + L)
    p = ref.resolve(n, small_params(n, ref.HALF))
    kinds, c = [], 0
    while c < L:                                                    # the background: short runs of every class
        w = int(rng.integers(1, 7))
        kinds += ["2210g"[int(rng.integers(0, 5))]] * w
        c += w
    m = np.stack([class_column(ch, n, p) for ch in kinds[:L]], axis=1)
    for i, col in enumerate(special_columns(n, p)):
        if i < L:
            m[:, i] = col
    placed = []
    bounds = [b for b in (64, W, 2 * W) if b < L]
    spots = [(b, (variant + i) % 4, b - PIECES[(variant + i) % 4][1]) for i, b in enumerate(bounds)]
    if not bounds:                                                  # no boundary: the pieces one after the other, as far as they fit
        at = 7
        for i in range(4):
            spots.append((None, (variant + i) % 4, at))
            at += len(PIECES[(variant + i) % 4][0]) + 1
    for b, k, start in spots:
        text = PIECES[k][0][:max(0, L - start)]
        for j, ch in enumerate(text):
            m[:, start + j] = class_column(ch, n, p)
        if text:
            placed.append((b, k, start, text))
    if variant % 2:
        m = m[rng.permutation(n)]                                   # the rows in another order: the majority vote sees another sequence
    return ref.gene_of(m), small_params(n, gaps), placed


# ---- 1. the bytes as k_gbclass and k_gbselect wrote them ----
@pytest.mark.parametrize("L", [1, 9, 63, 64, 65, W - 1, W, W + 1, 2 * W + 1])
@pytest.mark.parametrize("n", [1, 2, 3, 64, 65, 600])
def test_flags(gpu_ctx, n, L):
    seen_classes, fired = set(), np.zeros(5, dtype=int)
    for variant in range(4):
        for gaps in MODES:
            gene, params, placed = flags_gene(n, L, variant, gaps)
            p = ref.resolve(n, params)
            cls, gp = ref.classes(ref.matrix(gene), p)
            stages = ref.procedure(cls, gp, p)
            want = ref.flag_bytes(cls, gp, stages)
            if gaps == ref.HALF and n >= 3:                         # the planted runs are what they are meant to be, across their boundary
                for b, k, start, text in placed:
                    assert "".join("g" if g else str(c) for c, g in zip(cls[start:start + len(text)], gp[start:start + len(text)])) == text
                    assert b is None or start < b < start + len(text)
                if L > 2 * W:
                    assert [b for b, _, _, _ in placed] == [64, W, 2 * W]
                if L > 6:                                           # the thresholds, the tie and the alternating majority
                    assert cls[0] == 0 and cls[1] >= 1 and cls[3] == 2 and cls[5] == 0 and cls[6] == 1 and gp[4] == (n % 2 == 0)
                seen_classes |= set(cls)
                fired += ref.steps_exercised(stages)
            assert list(gpu_ctx.debug_gblocks_flags(gene, params)) == want, (variant, gaps)
            assert list(engine.gblocks_flags_host(gene, params)) == want, (variant, gaps)
    if n >= 3 and L >= W - 1:
        assert seen_classes == {0, 1, 2} and (fired > 0).all()       # the case tells the classes and the steps apart


@pytest.mark.parametrize("L", [LDS_COLS, LDS_COLS + 1, LDS_COLS + W + 3])
def test_flags_beyond_lds(gpu_ctx, L):
    """a gene of more than GB_LDS_COLS columns keeps its scan values in the scratch slice"""
    gene = ref.gene_of(ref.run_gene(np.random.default_rng(L), 7, L))
    for params in (None, {"b3": 3, "b4": 4, "b0": 4, "gaps": ref.NONE}):
        want = ref.flags(gene, params)
        assert 0 < sum(1 for f in want if f & ref.KEPT) < L
        assert list(gpu_ctx.debug_gblocks_flags(gene, params)) == want
        assert list(engine.gblocks_flags_host(gene, params)) == want


# ---- 2. gblocks_trim ----
# The seed was searched on the CPU with gblocks_ref (the first of 0, 1, 2, ... under which the assertions of _mixed_want hold)
MIXED_SEED = 0
MIXED_SHAPES = ((5, 300), (12, 700), (65, 1100))
_mixed = {}


def mixed_genes(seed=MIXED_SEED):
    rng = np.random.default_rng(seed)
    genes = [ref.gene_of(ref.run_gene(rng, n, L)) for n, L in MIXED_SHAPES]
    genes.append(ref.gene_of(np.full((4, 33), ord("A"), dtype=np.uint8)))                         # kept whole
    genes.append(ref.gene_of(ref.RESIDUES[rng.integers(0, 20, (9, 50))]))                         # emptied: no conserved column
    genes.append(ref.gene_of(np.array([[ord("A")], [ord("A")], [ord("-")]], dtype=np.uint8)))     # a single column
    return genes


def mixed_stage_cap(genes):
    """what the issue asks of the random genes, on the reference: all three classes, every step at work, 0 < nkept < L"""
    seen, fired, partly = set(), np.zeros(5, dtype=int), True
    for gene in genes[:len(MIXED_SHAPES)]:
        p = ref.resolve(len(gene[0]), None)
        cls, gp = ref.classes(ref.matrix(gene), p)
        stages = ref.procedure(cls, gp, p)
        seen |= set(cls)
        fired += ref.steps_exercised(stages)
        partly = partly and 0 < sum(stages[-1]) < len(cls)
    return seen == {0, 1, 2} and bool((fired > 0).all()) and partly


def _mixed_want():
    if not _mixed:
        _mixed["genes"] = mixed_genes()
        _mixed["want"] = [ref.trim(g) for g in _mixed["genes"]]
    return _mixed["genes"], _mixed["want"]


def test_gblocks_trim(gpu_ctx):
    genes, want = _mixed_want()
    assert mixed_stage_cap(genes)
    assert want[3]["nkept"] == 33 and want[4]["nkept"] == 0 and want[4]["ncols"] == 50 and (want[5]["ncols"], want[5]["nkept"]) == (1, 0)
    got = gpu_ctx.gblocks_trim(genes)
    again = gpu_ctx.gblocks_trim(genes)
    for g, (a, b, w) in enumerate(zip(got, again, want)):
        for key in ("kept_cols", "rows", "ncols", "nkept", "names", "gap_or_missing"):
            assert a[key] == w[key], (g, key)
        assert a == b, g                                            # two calls give identical bytes
    short = {"b3": 3, "b4": 2, "b0": 2, "gaps": ref.ALL}            # explicit parameters, genes in another order
    one = gpu_ctx.gblocks_trim([genes[5], genes[3], genes[0]], short)
    assert one == [ref.trim(g, short) for g in (genes[5], genes[3], genes[0])]
    assert one[1]["nkept"] == 33 and one[2]["kept_cols"] != want[0]["kept_cols"]
    with pytest.raises(engine.PmlError) as e:
        gpu_ctx.gblocks_trim(genes[:2], {"b1": 2})                  # b1 = 2 is not above half of 5 rows
    assert e.value.code == engine.EINVAL and "gene 0" in str(e.value)


def test_str_rows_and_the_mirror(gpu_ctx):
    rng = np.random.default_rng(3)
    names, rows = ref.gene_of(ref.run_gene(rng, 6, 200))
    rows = [r.decode() for r in rows]
    want = ref.trim((names, rows))
    assert 0 < want["nkept"] < 200 and gpu_ctx.gblocks_trim([(names, rows)])[0] == want
    out = tree_builder.MSATrimmer(gpu_ctx).trim(tree_builder.SequenceAlignment(names, rows, name="fam"))
    assert out.getName() == "fam_trim" and out.getTaxa() == names and out.rows == want["rows"]


# ---- 3. sub-batches under the HBM budget ----
def test_sub_batches(gpu_ctx, monkeypatch):
    rng = np.random.default_rng(6000)
    genes = [ref.gene_of(ref.run_gene(rng, 40, 6000)) for _ in range(4)]      # 6000 > GB_LDS_COLS: the scratch slices too
    assert 6000 > LDS_COLS
    free = gpu_ctx.gblocks_trim(genes)
    assert free == [ref.trim(g) for g in genes] and 0 < free[0]["nkept"] < 6000
    before, tbefore = gpu_ctx.gblocks_stats(), gpu_ctx.trim_stats()
    monkeypatch.setenv("PML_HBM_BUDGET_MB", "1")
    tight = gpu_ctx.gblocks_trim(genes)
    after, tafter = gpu_ctx.gblocks_stats(), gpu_ctx.trim_stats()
    assert tight == free
    assert after["class_launches"] - before["class_launches"] > 1 and after["select_launches"] - before["select_launches"] > 1
    assert tafter["gather_launches"] - tbefore["gather_launches"] > 1
    big = ref.gene_of(ref.RESIDUES[rng.integers(0, 20, (40, 60000))])
    with pytest.raises(engine.PmlError) as e:
        gpu_ctx.gblocks_trim([big])
    assert e.value.code == -4 and "MiB" in str(e.value) and "gene 0" in str(e.value)
    with pytest.raises(engine.PmlError) as e:                                   # the staged call is resident as a whole
        gpu_ctx.trim_pipeline(genes, True, None, engine.TRIM_GAP_UNIFORM, 0)
    assert e.value.code == -4 and "MiB" in str(e.value)
    monkeypatch.delenv("PML_HBM_BUDGET_MB")
    assert gpu_ctx.gblocks_trim(genes[:1]) == free[:1]                           # the same context goes on working


# ---- 4. the staged call ----
def stage_genes(seed, ntax=12, ngenes=10, ncols=150, noise=60, fast=0.35):
    """genes evolved slowly down one random tree over different taxon subsets, rows in shuffled order.  Gene 1 carries in its middle
    a block of `noise` fast columns evolved down ANOTHER tree, which the block selection removes; gene 4 is evolved down that other
    tree throughout, slowly, so its conserved columns stay."""
    rng = np.random.default_rng(seed)
    names = ["tx%03d" % i for i in range(ntax)]
    main, other = random_tree(rng, ntax), random_tree(rng, ntax)
    genes = []
    for g in range(ngenes):
        rows = evolve(rng, *(other if g == 4 else main), ntax, ncols + g, change=0.015, gaps=0.01)
        if g == 1:
            block = evolve(rng, *other, ntax, noise, change=fast, gaps=0.05)
            rows = [r[:ncols // 2] + f + r[ncols // 2:] for r, f in zip(rows, block)]
        lack = set(rng.choice(ntax, int(rng.integers(0, 3)), replace=False).tolist()) if g else set()
        keep = [t for t in range(ntax) if t not in lack]
        keep = [keep[i] for i in rng.permutation(len(keep))]
        genes.append(([names[t] for t in keep], [rows[t] for t in keep]))
    return genes


# The seed was searched on the CPU with the restatements (the first of 0, 1, 2, ... under which the assertions of _stage_case hold):
# no gene is emptied by a stage, no all-gap column reaches the uniform filter, and the Gblocks stage changes which gene the
# congruence filter drops
STAGE_SEED, STAGE_PERCENT = 8, 0.2
_stage = {}


def stage_reference(genes, p=STAGE_PERCENT):
    """the three restatements one after the other, and the last two without the first"""
    blocks = [ref.trim(g) for g in genes]
    uniform = trim_ref.trim_genes([(t["names"], t["rows"]) for t in blocks], trim_ref.UNIFORM)
    want = cref.congruence_filter([(t["names"], t["rows"]) for t in uniform], p)
    plain_trim = trim_ref.trim_genes(genes, trim_ref.UNIFORM)
    plain = cref.congruence_filter([(t["names"], t["rows"]) for t in plain_trim], p)
    return blocks, uniform, want, plain


def stage_case_holds(genes, blocks, uniform, want, plain):
    return (all(t["nkept"] > 0 for t in blocks) and blocks[1]["nkept"] < blocks[1]["ncols"] - 40 and all(0 < t["nkept"] < t["ncols"] for t in uniform)
            and want["keep"] != plain["keep"] and not plain["keep"][1] and want["keep"][1] and not all(want["keep"]))


def _stage_case():
    if not _stage:
        genes = stage_genes(STAGE_SEED)
        _stage["case"] = (genes,) + stage_reference(genes)
    return _stage["case"]


def _same_filter(got, want):
    assert got["names"] == want["names"] and got["n"] == want["n"] and got["cutoff"] == want["cutoff"]
    assert len(got["kept_splits"]) == len(want["kept"]) and set(got["kept_splits"]) == cref.kept_splits(want)
    for key in ("cost_sum", "mean_cost", "nsplits", "keep", "idx", "max_cost"):
        assert got[key] == want[key], key


def _same_dicts(a, b):
    assert a.keys() == b.keys()
    for key in a:
        if key == "kept_words":
            assert a[key].tobytes() == b[key].tobytes()
        else:
            assert a[key] == b[key], key


def test_trim_pipeline(gpu_ctx):
    genes, blocks, uniform, want, plain = _stage_case()
    assert stage_case_holds(genes, blocks, uniform, want, plain)    # the Gblocks stage changes the selection
    got = gpu_ctx.trim_pipeline(genes, True, None, engine.TRIM_UNIFORM, STAGE_PERCENT)
    _same_filter(got, want)                                         # the three restatements, one after the other
    assert got["gblocks"] == blocks and got["trimmed"] == uniform
    # the three calls one after the other, on the returned text: field for field
    one = gpu_ctx.gblocks_trim(genes)
    two = gpu_ctx.trim_columns([(t["names"], t["rows"]) for t in one], engine.TRIM_UNIFORM)
    three = gpu_ctx.congruence_filter([(t["names"], t["rows"]) for t in two], STAGE_PERCENT)
    assert one == got["gblocks"] and two == got["trimmed"]
    _same_dicts(three, {k: v for k, v in got.items() if k not in ("gblocks", "trimmed")})
    # two stages at a time
    a = gpu_ctx.trim_pipeline(genes, True, None, None, STAGE_PERCENT)
    assert a["gblocks"] == one and "trimmed" not in a
    _same_dicts(gpu_ctx.congruence_filter([(t["names"], t["rows"]) for t in one], STAGE_PERCENT), {k: v for k, v in a.items() if k != "gblocks"})
    b = gpu_ctx.trim_pipeline(genes, True, None, engine.TRIM_TOPOLOGICAL, 0)
    assert b == {"gblocks": one, "trimmed": gpu_ctx.trim_columns([(t["names"], t["rows"]) for t in one], engine.TRIM_TOPOLOGICAL)}
    assert b["trimmed"] == trim_ref.trim_genes([(t["names"], t["rows"]) for t in blocks], trim_ref.TOPOLOGICAL)
    c = gpu_ctx.trim_pipeline(genes, False, None, engine.TRIM_UNIFORM, STAGE_PERCENT)          # the chained call that exists, by the new door
    chained = gpu_ctx.trim_congruence_filter(genes, engine.TRIM_UNIFORM, STAGE_PERCENT)
    _same_dicts(c, chained)
    assert c["keep"] == plain["keep"] != got["keep"]
    explicit = {"b3": 4, "b4": 5, "b0": 5, "gaps": ref.NONE}
    d = gpu_ctx.trim_pipeline(genes, True, explicit, engine.TRIM_GAP_UNIFORM, 0)
    assert d["gblocks"] == [ref.trim(g, explicit) for g in genes] and d["gblocks"] != one
    assert d["trimmed"] == trim_ref.trim_genes([(t["names"], t["rows"]) for t in d["gblocks"]], trim_ref.GAP_UNIFORM)


def test_trim_pipeline_refusals(gpu_ctx):
    genes = _stage_case()[0][:3]
    noise = ref.gene_of(ref.RESIDUES[np.random.default_rng(5).integers(0, 20, (9, 50))], prefix="tx")      # the Gblocks stage empties it
    flat = (["tx000", "tx001", "tx002", "tx003"], ["A" * 12] * 4)                 # kept whole by Gblocks, emptied by the uniform filter
    assert ref.trim(noise)["nkept"] == 0 and ref.trim(flat)["nkept"] == 12
    for mode, percent in ((engine.TRIM_UNIFORM, 0), (None, 0.1), (engine.TRIM_UNIFORM, 0.1)):
        with pytest.raises(engine.PmlError) as e:
            gpu_ctx.trim_pipeline(genes + [noise], True, None, mode, percent)
        assert e.value.code == -2 and "gene 3" in str(e.value) and "Gblocks" in str(e.value) and "no columns left" in str(e.value)
    with pytest.raises(engine.PmlError) as e:
        gpu_ctx.trim_pipeline(genes[:1] + [flat] + genes[1:], True, None, engine.TRIM_UNIFORM, 0.1)
    assert e.value.code == -2 and "gene 1" in str(e.value) and "column filter" in str(e.value)
    only = gpu_ctx.trim_pipeline(genes + [noise, flat], True, None, None, 0)      # a single stage may empty a gene
    assert only == {"gblocks": gpu_ctx.gblocks_trim(genes + [noise, flat])} and only["gblocks"][3]["nkept"] == 0
    last = gpu_ctx.trim_pipeline(genes + [flat], True, None, engine.TRIM_UNIFORM, 0)              # the last stage may as well
    assert last["trimmed"][3]["nkept"] == 0 and last["gblocks"][3]["nkept"] == 12
    for args in ((False, None, None, 0), (True, None, 3, 0), (True, None, -2, 0), (True, None, None, -0.5), (True, None, None, float("nan")),
                 (True, {"b1": 1}, None, 0)):
        with pytest.raises(engine.PmlError) as e:
            gpu_ctx.trim_pipeline(genes, *args)
        assert e.value.code == engine.EINVAL, args
    assert gpu_ctx.trim_pipeline(genes, True, None, None, 0)["gblocks"] == [ref.trim(g) for g in genes]      # the context goes on working


# ---- 5. the tool ----
def test_tree_step_tool(gpu_ctx, tmp_path, monkeypatch, capsys):
    monkeypatch.syspath_prepend(os.path.join(ROOT, "tools"))
    import pepr_tree_step
    genes, blocks, uniform, want, _ = _stage_case()
    d = tmp_path / "alignments"
    d.mkdir()
    for i, (names, rows) in enumerate(genes):
        (d / ("fam%02d.fasta" % i)).write_text("".join(">%s\n%s\n" % (n, r) for n, r in zip(names, rows)))
    common = ["-alignment_dir", str(d), "-support_reps", "3", "-seed", "3", "--full-tree-method", "nj"]
    run = str(tmp_path / "all")
    pepr_tree_step.main(["-run_name", run, "-gblocks_trim", "-uniform_trim", "-congruence_filter", "-trim_percent", str(STAGE_PERCENT)] + common)
    out = capsys.readouterr().out
    lines = [l.split("\t") for l in open(run + ".gblocks.tsv").read().splitlines()]
    assert lines[0] == ["file", "columns", "kept"]
    assert lines[1:] == [["fam%02d.fasta" % i, str(t["ncols"]), str(t["nkept"])] for i, t in enumerate(blocks)]
    lines = [l.split("\t") for l in open(run + ".trim.tsv").read().splitlines()]
    assert lines[1:] == [["fam%02d.fasta" % i, str(t["ncols"]), str(t["nkept"])] for i, t in enumerate(uniform)]
    lines = [l.split("\t") for l in open(run + ".congruence.tsv").read().splitlines()]
    assert lines[1:] == [["fam%02d.fasta" % i, str(uniform[i]["nkept"]), str(want["cost_sum"][i]), str(want["mean_cost"][i]), str(int(want["keep"][i]))]
                         for i in range(len(genes))]
    dropped = [i for i, k in enumerate(want["keep"]) if not k]
    assert dropped and all("discarding set fam%02d.fasta" % i in out for i in dropped)
    kept = [(t["names"], t["rows"]) for t, k in zip(uniform, want["keep"]) if k]
    trees = gpu_ctx.nj_jackknife(kept, reps=3, seed=3, support_rule=engine.SUPPORT_DECORATOR)
    assert open(run + ".nwk").read() == trees["newick"] + "\n"      # the trees are built on the trimmed, kept genes
    # the block selection alone; a gene trimmed to nothing is dropped with a message
    noise = ref.RESIDUES[np.random.default_rng(5).integers(0, 20, (9, 50))]
    (d / "fam99.fasta").write_text("".join(">tx%03d\n%s\n" % (i, noise[i].tobytes().decode()) for i in range(9)))
    run2 = str(tmp_path / "blocks")
    pepr_tree_step.main(["-run_name", run2, "-gblocks_trim"] + common)
    out = capsys.readouterr().out
    assert open(run2 + ".gblocks.tsv").read().splitlines()[-1] == "fam99.fasta\t50\t0" and "dropping set fam99.fasta: no column left after -gblocks_trim" in out
    assert not os.path.exists(run2 + ".trim.tsv") and not os.path.exists(run2 + ".congruence.tsv")
    trees = gpu_ctx.nj_jackknife([(t["names"], t["rows"]) for t in blocks], reps=3, seed=3, support_rule=engine.SUPPORT_DECORATOR)
    assert open(run2 + ".nwk").read() == trees["newick"] + "\n"
    # with the emptied gene the stages run one after the other and give what they gave without it
    run3 = str(tmp_path / "both")
    pepr_tree_step.main(["-run_name", run3, "-gblocks_trim", "-congruence_filter", "-trim_percent", str(STAGE_PERCENT)] + common)
    out = capsys.readouterr().out
    assert "dropping set fam99.fasta" in out and not os.path.exists(run3 + ".trim.tsv")
    f = cref.congruence_filter([(t["names"], t["rows"]) for t in blocks], STAGE_PERCENT)
    lines = [l.split("\t") for l in open(run3 + ".congruence.tsv").read().splitlines()]
    assert lines[1:] == [["fam%02d.fasta" % i, str(blocks[i]["nkept"]), str(f["cost_sum"][i]), str(f["mean_cost"][i]), str(int(f["keep"][i]))]
                         for i in range(len(genes))]
