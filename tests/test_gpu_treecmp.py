"""Tree-set comparison on the device (treecmp.hip through pml_tree_compare and its two test doors) against the Python restatement
tests/treecmp_ref.py.  Every comparison is for equality: integers equal, sums and distances bit-equal as float64.view(int64) --
with every NaN taken as one value, as Java's doubleToLongBits takes them (the host's 0/0 and the device's differ in the sign bit).

The sets come from treecmp_ref.draw_set: one random tree perturbed by NNIs and SPRs, and in fixed places two identical trees, a
tree that shares nothing with tree 0 beyond the pendant branches (multifurcating where n allows, rooted at a bifurcating top level,
all lengths 0), tree 0's topology with other lengths, a multifurcating tree with missing lengths and a tree without lengths --
as many of these as T allows (T = 3 holds the first two kinds).  The parser admits no repeated split (a node with one child is
refused, as the Java's round trip destroys such a tree), so no set holds one; the restatement's own test covers that rule."""
import functools

import numpy as np
import pytest

from pepr_amd import engine, tree_builder
import treecmp_ref as ref

pytestmark = pytest.mark.gpu
RF = ("rf_legacy", "rf_bipartition", "rf_splits")
DIST = ("branch_dist", "discrepant_dist")
# k_tree_pairs takes 256 column trees per workgroup: T = 255 and 257 sit one under and one over it; 67 and 33 are ragged single tiles
SHAPES = [(4, 3), (5, 9), (12, 67), (64, 5), (65, 33), (129, 5), (257, 4), (512, 3)]


def bits(a):
    a = np.array(a, dtype=np.float64)
    a[np.isnan(a)] = np.nan                                         # one NaN
    return a.view(np.int64)


@functools.lru_cache(maxsize=None)
def the_set(n, T, use_lengths=True):
    texts = ref.draw_set(n, T, 1)
    return texts, ref.TreeSet(texts, use_lengths)


@functools.lru_cache(maxsize=None)
def full_reference(n, T, use_lengths=True, window=0):
    return the_set(n, T, use_lengths)[1].compare_all(window)


def assert_same(got, want, where=None):
    for k in RF:
        a, b = (got[k], want[k]) if where is None else (got[k][where], want[k][where])
        assert np.array_equal(a, b), k
    for k in DIST:
        a, b = (got[k], want[k]) if where is None else (got[k][where], want[k][where])
        assert np.array_equal(bits(a), bits(b)), k


@pytest.mark.parametrize("n", [4, 5, 63, 64, 65, 129, 257, 512])
def test_tree_splits_door(gpu_ctx, n):
    """the records in branch order, their words, lengths, normalisation and flags (TC_LAST included) against the restatement;
    equal splits get equal ids, different splits different ids, and the id is the index of the split's first record"""
    texts = ref.draw_set(n, 6, 2)
    rec = gpu_ctx.debug_tree_splits(texts)
    assert rec["names"] == sorted(ref.JTree(texts[0]).leaves) and rec["words"] == (1 if n <= 64 else 2 if n <= 128 else 4 if n <= 256 else 8)
    at = 0
    for t, text in enumerate(texts):
        want = ref.records(text)
        assert rec["first"][t] == at and rec["nreal"][t] == sum(1 for w in want if w[3] & ref.REAL)
        for k, w in enumerate(want):
            r = at + k
            assert rec["splits"][r] == w[0] and rec["flags"][r] == w[3], (t, k)
            assert bits(rec["length"][r]) == bits(w[1]) and bits(rec["length_norm"][r]) == bits(w[2]), (t, k)
        at += len(want)
    assert rec["first"][len(texts)] == at == len(rec["splits"])
    first = {}
    for r, s in enumerate(rec["splits"]):
        assert rec["split_id"][r] == first.setdefault(s, r), r


@pytest.mark.parametrize("n,T", SHAPES)
def test_whole_call(gpu_ctx, n, T):
    texts, _ = the_set(n, T)
    got = gpu_ctx.tree_compare(texts)
    assert_same(got, full_reference(n, T))
    for k in RF:
        assert (np.diag(got[k]) == 0).all() and np.array_equal(got[k], got[k].T)


@pytest.mark.parametrize("T", [255, 257])
def test_column_tile_boundary(gpu_ctx, T):
    """one tree under and one over the 256 columns of a workgroup; the restatement is run on five rows of the matrix"""
    texts, s = the_set(5, T)
    got = gpu_ctx.tree_compare(texts)
    for i in (0, 2, 100, 254, T - 1):
        for j in range(T):
            a, b = min(i, j), max(i, j)
            want = s.pair(a, b) if a != b else (0, 0, 0) + s.pair(a, a)[3:]
            assert tuple(int(got[k][i, j]) for k in RF) == tuple(want[:3]), (i, j)
            assert bits(got["branch_dist"][i, j]) == bits(want[3]) and bits(got["discrepant_dist"][i, j]) == bits(want[4]), (i, j)


def test_pair_sums_door(gpu_ctx):
    """the raw counts and the six sums of chosen pairs, the diagonal included"""
    texts, s = the_set(12, 67)
    pairs = [(0, 1), (0, 2), (0, 3), (2, 2), (2, 4), (3, 66), (4, 5), (10, 40), (65, 66), (66, 66)]
    counts, sums = gpu_ctx.debug_tree_pair_sums(texts, pairs)
    for p, (i, j) in enumerate(pairs):
        a, b = s.trees[i], s.trees[j]
        sh, sh_nt, da, da_nt, db, db_nt = ref.pair_counts(a, b)
        assert list(counts[p][[0, 1, 3, 4, 5, 6]]) == [sh, sh_nt, da, da_nt, db, db_nt], (i, j)
        assert counts[p][2] == len(s.resolved[i] & s.resolved[j])
        want = ref.branch_distance_sums(a, b) + ref.discrepant_distance_sums(a, b)
        assert np.array_equal(bits(sums[p]), bits(want)), (i, j, sums[p], want)
    with pytest.raises(engine.PmlError) as e:
        gpu_ctx.debug_tree_pair_sums(texts, [(3, 2)])
    assert e.value.code == -1


def test_without_lengths(gpu_ctx):
    texts, _ = the_set(12, 67, False)
    got = gpu_ctx.tree_compare(texts, use_lengths=False)
    assert_same(got, full_reference(12, 67, False))
    assert np.isnan(got["branch_dist"]).all() and np.isnan(got["discrepant_dist"]).all()


def test_rf_splits_is_pml_rf_distance(gpu_ctx):
    """the cross-check against code that exists without this feature: every pair of the (12, 67) set"""
    texts, _ = the_set(12, 67)
    got = gpu_ctx.tree_compare(texts, want=["rf_splits"])
    assert set(got) & set(RF + DIST) == {"rf_splits"}
    for i in range(67):
        for j in range(67):
            if i != j:
                assert got["rf_splits"][i, j] == engine.rf_distance(texts[i], texts[j]), (i, j)


def test_window(gpu_ctx):
    texts, _ = the_set(12, 67)
    full = gpu_ctx.tree_compare(texts)
    got = gpu_ctx.tree_compare(texts, window=10)
    i, j = np.indices((67, 67))
    band = np.abs(i - j) <= 10
    assert_same(got, full, band)
    assert_same(got, full_reference(12, 67), band)
    for k in RF:
        assert (got[k][~band] == -1).all()
    for k in DIST:
        assert np.isnan(got[k][~band]).all()
    # the Java's two band walkers
    assert tree_builder.rollingComparison(texts, ctx=gpu_ctx) == [int(full["rf_legacy"][k + 1, k]) for k in range(66)]
    w = tree_builder.compareSlidingWindow(texts, 10, ctx=gpu_ctx)
    assert [x[0] for x in w] == list(range(10, 67)) and w[5][1] == [(j, int(full["rf_legacy"][15, j])) for j in range(5, 15)]


def test_compare_one_and_the_mirrors(gpu_ctx):
    texts, _ = the_set(12, 67)
    got = gpu_ctx.tree_compare_one(texts[3], texts[4:30])
    want = ref.compare_one(texts[3], texts[4:30])
    assert_same(got, want)
    assert bits(tree_builder.getBranchDistance(texts[3], texts[9], ctx=gpu_ctx)) == bits(want["branch_dist"][5])
    assert bits(tree_builder.getDiscrepantBranchDistance(texts[3], texts[9], ctx=gpu_ctx)) == bits(want["discrepant_dist"][5])
    assert np.array_equal(tree_builder.compareAllvsAll(texts[:9], ctx=gpu_ctx)["rf_legacy"], full_reference(12, 67)["rf_legacy"][:9, :9])


def test_row_blocks(gpu_ctx, monkeypatch):
    """a budget that leaves room for 20 rows of pair outputs beside the records: the 67 rows come in four blocks, the last one
    ragged, and give the same bytes; a budget without room for one row is refused with the sizes"""
    texts, _ = the_set(12, 67)
    full = gpu_ctx.tree_compare(texts)
    assert full["row_blocks"] == 1 and full["row_bytes"] == 67 * 32
    monkeypatch.setenv("PML_HBM_BUDGET_MB", repr((full["resident_bytes"] + 20 * full["row_bytes"] + 8) / 1048576.0))
    got = gpu_ctx.tree_compare(texts)
    assert got["row_blocks"] == 4
    assert_same(got, full)
    monkeypatch.setenv("PML_HBM_BUDGET_MB", repr((full["resident_bytes"] + full["row_bytes"] // 2) / 1048576.0))
    with pytest.raises(engine.PmlError) as e:
        gpu_ctx.tree_compare(texts)
    assert e.value.code == -4 and str(full["row_bytes"]) in str(e.value)
    monkeypatch.setenv("PML_HBM_BUDGET_MB", "0")
    with pytest.raises(engine.PmlError) as e:
        gpu_ctx.tree_compare(texts)
    assert e.value.code == -4 and str(full["resident_bytes"]) in str(e.value)
    monkeypatch.delenv("PML_HBM_BUDGET_MB")
    assert_same(gpu_ctx.tree_compare(texts), full)                  # the same context goes on working


def test_refusals(gpu_ctx):
    """each decided on the host before any launch, each with its code and a pml_last_error text"""
    good = "((A:1,B:1):1,C:1,D:1);"
    rng = np.random.default_rng(1)
    big = ref.to_newick(ref.random_tree(rng, ["x%d" % i for i in range(513)]), lengths=False)
    for trees, code, word in [([good, "((A:1,B:1):1,C:1,E:1);"], -1, "leaf labels"), ([big, big], -1, "513"), ([], -1, "at least one tree"),
                              ([good, "((A:1,B:1"], -2, "tree 1"), ([good, "(A,B,C,D);"], -1, "top level"), ([good, "((A,B),(C),D);"], -1, "one child")]:
        with pytest.raises(engine.PmlError) as e:
            gpu_ctx.tree_compare(trees)
        assert e.value.code == code and word in str(e.value), (trees[:1], str(e.value))
    with pytest.raises(engine.PmlError) as e:
        gpu_ctx.tree_compare_one(good, ["((A:1,B:1):1,C:1,E:1);"])
    assert e.value.code == -1
    with pytest.raises(engine.PmlError) as e:
        gpu_ctx.tree_compare([good, good], window=-1)
    assert e.value.code == -1
    assert gpu_ctx.tree_compare([good, good])["rf_legacy"].tolist() == [[0, 0], [0, 0]]


def test_kernel_counter(gpu_ctx):
    before = gpu_ctx.kernel_stats()["treepairs"]["launches"]
    gpu_ctx.tree_compare(the_set(5, 9)[0])
    assert gpu_ctx.kernel_stats()["treepairs"]["launches"] == before + 1
