"""Column trimming on the device (`-uniform_trim`, MSATrimmer's three filters) against the restatement of the Java (trim_ref.py),
and the chained trim + congruence call against the two restatements one after the other.  Every comparison is for equality."""
import json
import os

import numpy as np
import pytest

from pepr_amd import engine, tree_builder
import congruence_ref as cref
import trim_ref as ref
from test_congruence_host import evolve, random_tree

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "trim_cases.json")))
ALPHABET = np.frombuffer(b"AC-?a\x80\xc1\xff", dtype=np.uint8)        # bytes from all four 64-bit quarters of the masks
MODES = (engine.TRIM_UNIFORM, engine.TRIM_GAP_UNIFORM, engine.TRIM_TOPOLOGICAL)


def random_matrix(rng, ntax, ncols, no_all_gap=False):
    """uint8 [ntax, ncols]: every column draws from its own few bytes, so that repeats and one-class columns are common"""
    m = np.empty((ntax, ncols), dtype=np.uint8)
    for c in range(ncols):
        k = int(rng.integers(1, len(ALPHABET) + 1))
        m[:, c] = ALPHABET[rng.choice(len(ALPHABET), k, replace=False)][rng.integers(0, k, ntax)]
        if no_all_gap and np.isin(m[:, c], (ref.GAP, ref.MISSING)).all():
            m[int(rng.integers(0, ntax)), c] = ord("C")
    return m


def gene_of(m, rng=None):
    """(names, rows as bytes); with rng the rows come in shuffled name order"""
    order = rng.permutation(m.shape[0]) if rng is not None else np.arange(m.shape[0])
    return (["t%03d" % i for i in order], [m[i].tobytes() for i in order])


def forced_column(text, ntax):
    """a hand-worked column of the golden file, tiled down ntax rows"""
    b = text.encode("latin-1")
    return np.frombuffer((b * (ntax // len(b) + 1))[:ntax], dtype=np.uint8)


# ---- 1. the flags as k_colclass wrote them ----
@pytest.mark.parametrize("ncols", [1, 15, 16, 17, 63, 64, 65, 257])
@pytest.mark.parametrize("ntax", [1, 2, 3, 64, 65, 600])
def test_flags(gpu_ctx, ntax, ncols):
    rng = np.random.default_rng(1000 * ntax + ncols)
    m = random_matrix(rng, ntax, ncols)
    forced = [forced_column(c["column"], ntax) for c in GOLD["cases"]]
    start = 64 - len(forced) // 2 if ncols > 64 else 0             # on both sides of the 64-column boundary where there is one
    planted = 0
    for i, col in enumerate(forced):
        if start + i < ncols:
            m[:, start + i] = col
            planted += 1
    if ncols == 257:
        assert planted == len(forced) and start < 63 and start + planted > 65
    gene = gene_of(m, rng)
    want = [ref.flags(col) for col in ref.columns(gene)]
    got = gpu_ctx.debug_column_flags(gene)
    assert list(got) == want
    assert list(engine.trim_column_flags_host(gene)) == want       # the same function on the host
    if ntax >= 3 and ncols >= 64:
        assert len(set(want)) >= 4                                  # the case tells the values apart


# ---- 2. trim_columns ----
def _seven_genes():
    rng = np.random.default_rng(77)
    genes = [gene_of(random_matrix(rng, nt, nc, no_all_gap=True), rng) for nt, nc in ((5, 100), (64, 257), (65, 64), (600, 17))]
    every = np.array([list(b"AACCDDA")] * 40, dtype=np.uint8).T.copy()           # three classes, each twice: kept by all three
    every[:, ::2] = every[::-1, ::2]
    genes.append(gene_of(every, rng))
    genes.append(gene_of(np.full((4, 33), ord("A"), dtype=np.uint8)))             # one class: dropped by all three
    genes.append(gene_of(np.array([[ord("A")], [ord("C")], [ord("-")]], dtype=np.uint8)))     # a single column, kept by the first two
    return genes


_seven = {}


def _seven_want(mode):
    if not _seven:
        _seven["genes"] = _seven_genes()
    if mode not in _seven:
        _seven[mode] = ref.trim_genes(_seven["genes"], mode)
    return _seven["genes"], _seven[mode]


@pytest.mark.parametrize("mode", MODES, ids=["uniform", "gap_uniform", "topological"])
def test_trim_columns(gpu_ctx, mode):
    genes, want = _seven_want(mode)
    assert len(genes) == 7 and want[4]["nkept"] == 40 and want[5]["nkept"] == 0 and want[6]["ncols"] == 1
    assert want[6]["nkept"] == (0 if mode == engine.TRIM_TOPOLOGICAL else 1)
    assert all(0 < w["nkept"] < w["ncols"] for w in want[:4])
    got = gpu_ctx.trim_columns(genes, mode)
    again = gpu_ctx.trim_columns(genes, mode)
    for g, (a, b, w) in enumerate(zip(got, again, want)):
        for key in ("kept_cols", "rows", "ncols", "nkept", "names"):
            assert a[key] == w[key], (g, key)
        cells = np.frombuffer(b"".join(genes[g][1]), dtype=np.uint8)
        assert a["gap_or_missing"] == w["gap_or_missing"] == int(np.isin(cells, (ref.GAP, ref.MISSING)).sum()), g
        assert a == b, g                                            # two calls give identical bytes
    assert all(isinstance(r, bytes) for r in got[0]["rows"])


def test_str_rows_and_the_mirror(gpu_ctx):
    gene = (["x", "y", "z", "w"], ["AAAC", "AAAC", "ACCD", "CC-D"])
    assert gpu_ctx.trim_columns([gene], engine.TRIM_UNIFORM)[0]["rows"] == ["A", "A", "C", "-"]
    m = tree_builder.MSATrimmer(gpu_ctx)
    aln = tree_builder.SequenceAlignment(*gene, name="fam")
    out = m.trimTopologicallyUninformativeColumns(aln)
    assert out.rows == ["AC", "AC", "CD", "CD"] and out.getName() is None and out.getTaxa() == gene[0]
    assert m.trimUniformColumns(aln).getName() == "fam_ui" and m.trimUniformativeColumns(aln).rows == gene[1]


def test_all_gap_column_is_refused_under_uniform(gpu_ctx):
    ok = (["a", "b", "c"], ["ACA", "CCA", "-DA"])
    bad = (["a", "b", "c", "d"], ["ACDAC-A", "ACDAC?A", "CADCA-C", "CCDDA?-"])
    with pytest.raises(engine.PmlError) as e:
        gpu_ctx.trim_columns([ok, bad], engine.TRIM_UNIFORM)
    assert e.value.code == -2 and "gene 1" in str(e.value) and "column 5" in str(e.value)
    with pytest.raises(ValueError):
        ref.trim(bad, ref.UNIFORM)
    for mode in (engine.TRIM_GAP_UNIFORM, engine.TRIM_TOPOLOGICAL):             # the other two drop it
        got = gpu_ctx.trim_columns([ok, bad], mode)
        assert [g["kept_cols"] for g in got] == [w["kept_cols"] for w in ref.trim_genes([ok, bad], mode)] and 5 not in got[1]["kept_cols"]
    assert gpu_ctx.debug_column_flags(bad)[5] == 8


# ---- 3. sub-batches under the HBM budget ----
def test_sub_batches(gpu_ctx, monkeypatch):
    rng = np.random.default_rng(6000)
    letters = np.frombuffer(b"ACDE-", dtype=np.uint8)
    genes = [gene_of(letters[rng.choice(5, (40, 6000), p=[0.93, 0.03, 0.02, 0.015, 0.005])]) for _ in range(6)]
    free = gpu_ctx.trim_columns(genes, engine.TRIM_UNIFORM)
    assert [f["kept_cols"] for f in free] == [t["kept_cols"] for t in ref.trim_genes(genes, ref.UNIFORM)] and 0 < free[0]["nkept"] < 6000
    before = gpu_ctx.trim_stats()
    monkeypatch.setenv("PML_HBM_BUDGET_MB", "1")
    tight = gpu_ctx.trim_columns(genes, engine.TRIM_UNIFORM)
    after = gpu_ctx.trim_stats()
    assert tight == free
    assert after["class_launches"] - before["class_launches"] > 1 and after["gather_launches"] - before["gather_launches"] > 1
    big = gene_of(letters[rng.choice(5, (40, 60000))])
    with pytest.raises(engine.PmlError) as e:
        gpu_ctx.trim_columns([big], engine.TRIM_UNIFORM)
    assert e.value.code == -4 and "MiB" in str(e.value) and "gene 0" in str(e.value)
    with pytest.raises(engine.PmlError) as e:                                   # the chained call is resident as a whole
        gpu_ctx.trim_congruence_filter(genes, engine.TRIM_UNIFORM, 0.1)
    assert e.value.code == -4 and "MiB" in str(e.value)
    monkeypatch.delenv("PML_HBM_BUDGET_MB")
    assert gpu_ctx.trim_columns(genes[:1], engine.TRIM_UNIFORM) == free[:1]      # the same context goes on working


# ---- 4. the chained call ----
def chain_genes(seed, ntax, ngenes, ncols, block):
    """genes evolved down one random tree (gene 1 down another), over different taxon subsets, rows in shuffled order; most lack
    one to three taxa, the last covers only 6.  Genes 1 and 4 end in a block of `block` columns that -uniform_trim drops: one
    residue throughout, or two residues without a gap"""
    rng = np.random.default_rng(seed)
    names = ["tx%03d" % i for i in range(ntax)]
    main, other = random_tree(rng, ntax), random_tree(rng, ntax)
    genes = []
    for g in range(ngenes):
        rows = evolve(rng, *(other if g == 1 else main), ntax, ncols + g)
        lack = set(rng.choice(ntax, int(rng.integers(0, 4)), replace=False).tolist()) if g else set()
        keep = [t for t in range(ntax) if t not in lack] if g < ngenes - 1 else sorted(rng.choice(ntax, 6, replace=False).tolist())
        keep = [keep[i] for i in rng.permutation(len(keep))]
        rows = [rows[t] for t in keep]
        if g in (1, 4):
            cut = int(rng.integers(1, len(keep)))
            rows = [r + ("A" * (block // 2)) + ("G" if i < cut else "L") * (block - block // 2) for i, r in enumerate(rows)]
        genes.append(([names[t] for t in keep], rows))
    return genes


# ntax: (seed, genes, columns, block, trim_percent).  The seeds were searched on the CPU with the two restatements: no gene has an all-gap column
# or trims to nothing, and the planted gene 1 is kept by the untrimmed filter and dropped by the trimmed one
CHAIN = {12: (1, 20, 60, 240, 0.1), 65: (1, 10, 30, 120, 0.2)}
_chain = {}


def _chain_case(ntax):
    if ntax not in _chain:
        seed, ngenes, ncols, block, p = CHAIN[ntax]
        genes = chain_genes(seed, ntax, ngenes, ncols, block)
        trimmed = ref.trim_genes(genes, ref.UNIFORM)
        want = cref.congruence_filter([(t["names"], t["rows"]) for t in trimmed], p)
        _chain[ntax] = (genes, trimmed, want, cref.congruence_filter(genes, p))
    return _chain[ntax]


def _same_filter(got, want):
    assert got["names"] == want["names"] and got["n"] == want["n"] and got["cutoff"] == want["cutoff"]
    assert len(got["kept_splits"]) == len(want["kept"]) and set(got["kept_splits"]) == cref.kept_splits(want)
    for key in ("cost_sum", "mean_cost", "nsplits", "keep", "idx", "max_cost"):
        assert got[key] == want[key], key


@pytest.mark.parametrize("ntax", sorted(CHAIN))
def test_chained_call(gpu_ctx, ntax):
    genes, trimmed, want, untrimmed = _chain_case(ntax)
    p = CHAIN[ntax][4]
    assert len(want["names"]) == ntax and any(want["cost_sum"]) and len({frozenset(g[0]) for g in genes}) > 3
    assert untrimmed["keep"][1] and not want["keep"][1]            # the trim changes the selection of the planted gene
    got = gpu_ctx.trim_congruence_filter(genes, engine.TRIM_UNIFORM, p)
    _same_filter(got, want)                                         # the two restatements, one after the other
    for a, w in zip(got["trimmed"], trimmed):
        assert {k: a[k] for k in w} == w
    # the two calls one after the other, on the returned text: field for field
    two = gpu_ctx.trim_columns(genes, engine.TRIM_UNIFORM)
    assert two == got["trimmed"]
    f = gpu_ctx.congruence_filter([(t["names"], t["rows"]) for t in two], p)
    assert f.keys() | {"trimmed"} == got.keys()
    for key in f:
        if key == "kept_words":
            assert f[key].tobytes() == got[key].tobytes()
        else:
            assert f[key] == got[key], key
    plain = gpu_ctx.congruence_filter(genes, p)                   # what the filter said before the trim existed
    assert plain["keep"] == untrimmed["keep"] and plain["keep"] != got["keep"]


def test_chained_call_refusals(gpu_ctx):
    ok = (["a", "b", "c", "d"], ["ACA", "CCA", "-DA", "ADC"])
    gone = (["a", "b", "c"], ["AAC", "AAC", "ACC"])                 # every column is two gap-free classes or one: trimmed to nothing
    assert ref.trim(gone, ref.UNIFORM)["nkept"] == 0
    with pytest.raises(engine.PmlError) as e:
        gpu_ctx.trim_congruence_filter([ok, gone], engine.TRIM_UNIFORM, 0.1)
    assert e.value.code == -2 and "gene 1" in str(e.value)
    with pytest.raises(engine.PmlError) as e:
        gpu_ctx.trim_congruence_filter([ok], engine.TRIM_UNIFORM, 0)
    assert e.value.code == engine.EINVAL
    with pytest.raises(engine.PmlError) as e:
        gpu_ctx.trim_columns([ok], 3)
    assert e.value.code == engine.EINVAL
    r = gpu_ctx.trim_congruence_filter([ok], engine.TRIM_GAP_UNIFORM, 0.5)      # the same context goes on working; a repeated name below
    assert r["trimmed"][0]["kept_cols"] == [0, 1, 2] and r["keep"] == [True]
    twice = (["a", "b", "a", "c"], ["ACA", "CCA", "-DA", "ADC"])
    got = gpu_ctx.trim_congruence_filter([twice, ok], engine.TRIM_GAP_UNIFORM, 0.5)
    t = gpu_ctx.trim_columns([twice, ok], engine.TRIM_GAP_UNIFORM)
    assert got["trimmed"] == t and t[0]["rows"] == twice[1]
    f = gpu_ctx.congruence_filter([(x["names"], x["rows"]) for x in t], 0.5)
    assert (f["cost_sum"], f["mean_cost"], f["nsplits"], f["keep"]) == (got["cost_sum"], got["mean_cost"], got["nsplits"], got["keep"])


# ---- 5. the tool ----
def test_tree_step_tool(gpu_ctx, tmp_path, monkeypatch, capsys):
    monkeypatch.syspath_prepend(os.path.join(ROOT, "tools"))
    import pepr_tree_step
    genes, trimmed, want, _ = _chain_case(12)
    d = tmp_path / "alignments"
    d.mkdir()
    for i, (names, rows) in enumerate(genes):
        (d / ("fam%02d.fasta" % i)).write_text("".join(">%s\n%s\n" % (n, r) for n, r in zip(names, rows)))
    run = str(tmp_path / "both")
    pepr_tree_step.main(["-run_name", run, "-alignment_dir", str(d), "-support_reps", "3", "-seed", "3", "--full-tree-method", "nj",
                         "-uniform_trim", "-congruence_filter", "-trim_percent", "0.1"])
    out = capsys.readouterr().out
    lines = [l.split("\t") for l in open(run + ".trim.tsv").read().splitlines()]
    assert lines[0] == ["file", "columns", "kept"]
    assert lines[1:] == [["fam%02d.fasta" % i, str(t["ncols"]), str(t["nkept"])] for i, t in enumerate(trimmed)]
    lines = [l.split("\t") for l in open(run + ".congruence.tsv").read().splitlines()]
    assert lines[1:] == [["fam%02d.fasta" % i, str(trimmed[i]["nkept"]), str(want["cost_sum"][i]), str(want["mean_cost"][i]), str(int(want["keep"][i]))]
                         for i in range(len(genes))]
    assert "discarding set fam01.fasta" in out
    kept = [(t["names"], t["rows"]) for t, k in zip(trimmed, want["keep"]) if k]
    trees = gpu_ctx.nj_jackknife(kept, reps=3, seed=3, support_rule=engine.SUPPORT_DECORATOR)
    assert open(run + ".nwk").read() == trees["newick"] + "\n"      # the trees are built on the trimmed, kept genes
    assert open(run + ".sup").read() == "\n".join(trees["support_trees"]) + "\n"
    # the trim alone; a gene trimmed to nothing is dropped with a message
    (d / "fam99.fasta").write_text(">tx000\nAAC\n>tx001\nAAC\n>tx002\nACC\n")
    run2 = str(tmp_path / "trim")
    pepr_tree_step.main(["-run_name", run2, "-alignment_dir", str(d), "-support_reps", "3", "-seed", "3", "--full-tree-method", "nj", "-uniform_trim"])
    out = capsys.readouterr().out
    assert open(run2 + ".trim.tsv").read().splitlines()[-1] == "fam99.fasta\t3\t0" and "dropping set fam99.fasta" in out
    assert not os.path.exists(run2 + ".congruence.tsv")
    trees = gpu_ctx.nj_jackknife([(t["names"], t["rows"]) for t in trimmed], reps=3, seed=3, support_rule=engine.SUPPORT_DECORATOR)
    assert open(run2 + ".nwk").read() == trees["newick"] + "\n"
