"""The multiple alignment on the device (csrc/msa.hip) against the host twin and, at the boundaries, tests/msa_ref.py: scores, paths,
rows and merges are equal, never just close.  Every class through the test door at its strip, group and pass boundaries, planted
gaps there, other costs and tables, the bound, a mixed batch of forty sets with its launch counts and sub-batches, and the whole
step from genome files to trimmed alignments."""
import os
import sys

import numpy as np
import pytest

from pepr_amd import engine, tree_builder
import msa_ref as ref
import sw_ref
from sw_ref import PLAIN, gap_subjects, mutate, planted_families, random_protein

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIM = engine.msa_limits()
T = LIM["strip"]
EINVAL, ENOMEM = -1, -4
SHAPES = [(1, 1), (1, 2), (2, 1), (2, 2), (5, 1), (1, 5), (2, 5), (5, 2), (5, 5)]


def same(got, want):
    assert got["score"] == want["score"]
    assert got["path"] == want["path"]
    assert got["rows"] == want["rows"]
    assert got["merges"] == want["merges"]


def check(ctx, X, Y, cls=-1, with_ref=True, **opts):
    got = ctx.msa_profile_align(X, Y, force_class=cls, **opts)
    same(got, engine.msa_profile_align_host(X, Y, **opts))
    if with_ref:
        score, path, rows = ref.profile_align(X, Y, opts.get("table"), opts.get("gap_open", 11), opts.get("gap_extend", 1))
        assert (got["score"], got["path"], got["rows"]) == (score, path, rows)
    return got


@pytest.mark.parametrize("cls", [0, 1, 2])
def test_profile_align_at_the_boundaries(gpu_ctx, cls):
    L, rows = LIM["lanes"][cls], LIM["rows"][cls]
    assert rows == L * T
    rng = np.random.default_rng(70 + cls)
    k = 0
    for LX in [1, T - 1, T, T + 1, rows - 1, rows] + ([rows + 1, 2 * rows + 1] if cls == 2 else []):
        for LY in (1, 2, 63, 64, 65):
            nX, nY = SHAPES[k % len(SHAPES)]
            k += 1
            check(gpu_ctx, ref.random_profile(rng, nX, LX), ref.random_profile(rng, nY, LY), cls)
    # planted gaps at the strip boundaries and, in the widest class, at the pass boundaries: the direction words there are read
    long_x = random_protein(rng, (2 * rows + 40) if cls == 2 else rows, PLAIN)
    for at in [T, 5 * T, rows - T] + ([rows, 2 * rows] if cls == 2 else []):
        for kind, piece in zip("21", gap_subjects(long_x, at)):                    # residues cut out: X's columns alone; put in: Y's
            got = check(gpu_ctx, [long_x], [piece], cls)
            core = "".join(str(p) for p in got["path"]).strip("2")
            assert core.strip("0") and set(core) == {"0", kind}, core       # a gap inside, not only X's free ends
            got = check(gpu_ctx, [long_x, mutate(rng, long_x)], [piece, mutate(rng, piece)], cls, with_ref=cls < 2)
    if cls < 2:                                                                    # X longer than the class's one pass
        with pytest.raises(engine.PmlError) as e:
            gpu_ctx.msa_profile_align([random_protein(rng, rows + 1, PLAIN)], ["ACD"], force_class=cls)
        assert e.value.code == EINVAL and "does not fit class %d" % cls in str(e.value)


def test_other_costs_tables_and_class_by_length(gpu_ctx):
    rng = np.random.default_rng(9)
    mild, wild = ref.asym_tables()
    edge = np.full((24, 24), -127, dtype=np.int64)
    edge[np.diag_indices(24)] = 127
    for LX, LY in ((37, 52), (130, 64), (300, 41)):                                # one per class, chosen by length
        for nX, nY in ((1, 1), (2, 5), (5, 2)):
            X, Y = ref.random_profile(rng, nX, LX), ref.random_profile(rng, nY, LY)
            check(gpu_ctx, X, Y, gap_open=3, gap_extend=2)
            for t in (mild, wild, wild.T.copy(), edge):
                check(gpu_ctx, X, Y, table=t, with_ref=LX < 100)
                check(gpu_ctx, Y, X, table=t, with_ref=LX < 100)


def test_the_bound_on_the_device_side(gpu_ctx):
    rng = np.random.default_rng(8)
    X, Y = ref.random_profile(rng, 5, 45, 0.1), ref.random_profile(rng, 5, 43, 0.1)
    table = sw_ref.blosum62()
    go = max(g for g in range(2 ** 19, 2 ** 20) if ref.bound(5, 5, 45, 43, table, g, 1) < 2 ** 30)
    check(gpu_ctx, X, Y, gap_open=go)
    with pytest.raises(engine.PmlError) as e:
        gpu_ctx.msa_profile_align(X, Y, gap_open=go + 1)
    assert e.value.code == EINVAL and "set 0" in str(e.value) and "2^30" in str(e.value)
    fam = ref.family(rng, 12, 300)
    with pytest.raises(engine.PmlError) as e:
        gpu_ctx.msa_align([["ACDE", "ACDF"], fam], gap_open=2 ** 20)
    assert e.value.code == EINVAL and "set 1" in str(e.value) and "2^30" in str(e.value)


@pytest.fixture(scope="module")
def forty_sets():
    rng = np.random.default_rng(40)
    sets = []
    for k in range(40):
        n = 1 + k % 12
        length = int(rng.integers(15, 60)) if k % 7 else int(rng.integers(140, 330))     # all three classes
        sets.append(ref.family(rng, n, length, deletions=1, truncate=n >= 3, alphabet=sw_ref.ALPHABET if k % 3 == 0 else PLAIN))
    return sets, engine.msa_align_host(sets)


def delta(ctx, f):
    a = ctx.msa_stats()
    out = f()
    b = ctx.msa_stats()
    return out, {k: ([y - x for x, y in zip(a[k], b[k])] if isinstance(a[k], list) else b[k] - a[k]) for k in a if k != "ms"}


def test_forty_sets_in_one_call(gpu_ctx, forty_sets, monkeypatch):
    sets, want = forty_sets
    got, d = delta(gpu_ctx, lambda: gpu_ctx.msa_align(sets))
    assert got == want
    for seqs, r in zip(sets, got):
        assert [ref.degap(x) for x in r["rows"]] == [ref.clean(s) for s in seqs]
    depth = [max([m[2] for m in r["merges"]] or [0]) for r in want]
    deepest = int(np.argmax(depth))
    alone, d1 = delta(gpu_ctx, lambda: gpu_ctx.msa_align([sets[deepest]]))
    assert alone == [want[deepest]]
    print("forty sets:", d, "the deepest alone:", d1)
    assert d["launches"] == d1["launches"] and d["levels"] == d1["levels"] == max(depth) and d["sub_batches"] == d1["sub_batches"]
    assert d["launches"] == [max(depth) + 1, max(depth), max(depth), max(depth)]      # k_msa_counts once a call with the first
    assert d["merges"] == sum(len(s) - 1 for s in sets) and d1["merges"] == len(sets[deepest]) - 1
    # a scratch budget that splits the levels into sub-batches: the same result
    monkeypatch.setenv("PML_MSA_SCRATCH_BYTES", "200000")
    split, d2 = delta(gpu_ctx, lambda: gpu_ctx.msa_align(sets))
    assert split == want and d2["sub_batches"] > d2["levels"] and d2["launches"][1] == d2["sub_batches"]
    # a merge above the budget is refused, the set named
    monkeypatch.setenv("PML_MSA_SCRATCH_BYTES", "4096")
    with pytest.raises(engine.PmlError) as e:
        gpu_ctx.msa_align(sets)
    assert e.value.code == ENOMEM and "set " in str(e.value) and "scratch budget" in str(e.value)


def test_the_whole_step_from_genome_files(gpu_ctx, tmp_path):
    import pepr_align_sets
    import pepr_tree_step
    genomes = planted_families(ngenomes=5)
    files = []
    for g, genome in enumerate(genomes):
        path = tmp_path / ("genome%d.faa" % g)
        path.write_text("".join(">%s\n%s\n" % (title, res) for title, res in genome))
        files.append(str(path))
    search = tree_builder.HomologySearch(files, evalue=0.1, run_name="m1", ctx=gpu_ctx, out_dir=str(tmp_path))
    hg = tree_builder.HomologGroups(search.getResults(), files, ctx=gpu_ctx, run_name="m1", out_dir=str(tmp_path))
    hg.run()
    set_files = hg.getSetFiles()
    assert len(set_files) == 3
    sets = [tree_builder.HomologySearch.readGenome(p) for p in set_files]
    aligner = tree_builder.MultipleSequenceAligner(ctx=gpu_ctx)
    alignments = aligner.getMSAs(sets, names=["set_%d" % k for k in range(3)])
    host = engine.msa_align_host([[r for _, r in s] for s in sets])
    for a, s, h in zip(alignments, sets, host):
        assert a.getName().endswith("_align") and a.getTaxa() == [t for t, _ in s] and a.rows == h["rows"] and len(a.rows) == 5
        trimmed = tree_builder.MSATrimmer(gpu_ctx).trim(tree_builder.SequenceAlignment(["t%d" % i for i in range(5)], a.rows, a.getName()))
        assert trimmed.getName().endswith("_align_trim") and 0 < trimmed.getLength() <= a.getLength()
    staged = gpu_ctx.trim_pipeline([(["t%d" % i for i in range(5)], a.rows) for a in alignments])      # pml_trim_pipeline accepts the alignments
    assert len(staged["gblocks"]) == 3
    out = str(tmp_path / "aligned")
    assert pepr_align_sets.main(["-sets"] + set_files + ["-genome_file"] + files + ["-o", out], ctx=gpu_ctx) == 0
    produced = sorted(os.listdir(out))
    assert produced == ["set_%d_align.faa" % k for k in range(3)]
    for name, h in zip(produced, host):
        names, rows = pepr_tree_step.read_fasta(os.path.join(out, name))
        assert sorted(names) == ["genome_%d" % g for g in range(5)] and rows == h["rows"]
