"""Weighted tree selection tests on the device (k_rell_pairsd, the weighted arm of k_rell, pml_rell_tests_weighted,
pml_tree_tests_weighted, the runConsel mirror's full table) against the numpy restatement in tests/rell_wref.py.

1 / sigma is compared to 1e-12 relative (the device sums in plain double in its own order, the reference in longdouble); the
statistics are integer counts and are compared EXACTLY.  That is licensed by tests/test_tree_tests_weighted_host.py: for every
(seed, shape) used here the reference holds no comparison within 1e-9 of a tie, so the last bits of sigma cannot flip one."""
import numpy as np
import pytest

import rell_ref
import rell_wref
import util
from pepr_amd import engine, synth, tree_builder as tb

pytestmark = pytest.mark.gpu

PLAIN = ("Y", "bp", "kh", "sh")


def _same_plain(a, b, tag):
    """the plain arm's results, bit for bit"""
    for f in PLAIN:
        assert a[f].tobytes() == b[f].tobytes(), (tag, f)


@pytest.mark.parametrize("N,T", rell_wref.SIGMA_CASES)
def test_pairsd_through_the_door(gpu_ctx, N, T):
    X = rell_wref.table(N, T, 77 * N + T)
    got = gpu_ctx.debug_rell(X, [N], 37, seed=1, weighted=True)["inv_sigma"]
    ref = rell_wref.inv_of(rell_wref.pair_sigma(X))
    assert got.shape == (T, T)
    assert np.array_equal(got, got.T)                                                  # exact symmetry
    assert np.all(np.diag(got) == 0.0)
    assert np.array_equal(got == 0.0, ref == 0.0)                                      # exact zeros where defined, and nowhere else
    if N == 1:
        assert not got.any()
    if T >= 4 and N > 1:
        assert got[0, 3] == 0.0 and got[0, 1] > 0 and got[3, 1] == got[0, 1]           # identical columns: excluded, and alike to the rest
    nz = ref > 0
    if nz.any():
        err = np.abs(got[nz] - ref[nz]) / ref[nz]
        print("N %d T %d: max relative error of 1 / sigma %.3g" % (N, T, err.max()))
        assert err.max() <= 1e-12


@pytest.mark.parametrize("K,B,T", rell_wref.COUNT_CASES)
def test_counts_through_the_door(gpu_ctx, K, B, T):
    N = rell_wref.COUNT_N
    X, nd, seed, Y, ref = rell_wref.case(N, T, K, B)
    tag = (N, T, K, B)
    plain = {p: gpu_ctx.debug_rell(X, nd, B, seed=seed, path=p) for p in (1, 2)}
    assert np.array_equal(plain[1]["Y"], Y)
    given = gpu_ctx.debug_rell(X, nd, B, seed=seed, path=1, inv_sigma=ref["inv_sigma"])
    lds = gpu_ctx.debug_rell(X, nd, B, seed=seed, path=1, weighted=True)
    glb = gpu_ctx.debug_rell(X, nd, B, seed=seed, path=2, weighted=True)
    assert given["path"] == 1 and lds["path"] == 1 and glb["path"] == 2
    assert np.array_equal(given["inv_sigma"], ref["inv_sigma"])                        # the matrix that was used: the one given
    for got in (given, lds, glb):
        assert np.array_equal(got["wkh"], ref["wkh"]) and np.array_equal(got["wsh"], ref["wsh"]), (tag, got["wkh"], ref["wkh"], got["wsh"], ref["wsh"])
    assert lds["inv_sigma"].tobytes() == glb["inv_sigma"].tobytes()
    _same_plain(given, plain[1], tag)
    _same_plain(lds, plain[1], tag)
    _same_plain(glb, plain[2], tag)
    if T == 2:                                                                          # a single pair: the sigma cancels
        assert np.array_equal(lds["wkh"], plain[1]["kh"]) and np.array_equal(lds["wsh"], plain[1]["kh"])


def test_degenerate_cases(gpu_ctx):
    # N = 1: every sigma is 0, every weighted p-value 1
    X, nd, seed, Y, ref = rell_wref.case(1, 5, 1, 37)
    got = gpu_ctx.debug_rell(X, nd, 37, seed=seed, weighted=True)
    assert not got["inv_sigma"].any() and np.all(got["wkh"] == 37) and np.all(got["wsh"] == 37)
    _same_plain(got, gpu_ctx.debug_rell(X, nd, 37, seed=seed), "N = 1")
    w = gpu_ctx.rell_tests(X, scales=[1.0], reps=37, seed=seed, weighted=True)
    assert np.all(w["wkh"] == 1.0) and np.all(w["wsh"] == 1.0) and np.all(w["wkh_other"] == -1) and not w["sigma"].any()
    # N = 7
    X, nd, seed, Y, ref = rell_wref.case(7, 5, 1, 37)
    got = gpu_ctx.debug_rell(X, nd, 37, seed=seed, weighted=True)
    assert np.array_equal(got["wkh"], ref["wkh"]) and np.array_equal(got["wsh"], ref["wsh"])
    # trees 0 and 3 are identical: that pair is excluded, their other pairs still count
    X, nd, seed, Y, ref = rell_wref.case(rell_wref.COUNT_N, 5, 1, 1000)
    got = gpu_ctx.debug_rell(X, nd, 1000, seed=seed, weighted=True)
    assert got["inv_sigma"][0, 3] == 0.0 and np.count_nonzero(got["inv_sigma"][0]) == 3
    assert got["wsh"][0] == got["wsh"][3] == ref["wsh"][0] and got["wkh"][0] == got["wkh"][3] == ref["wkh"][0]
    assert 0 < ref["wsh"][1] < 1000                                                     # a count that says something
    # a matrix that excludes more: tree 4 has no pair left -> it counts every replicate, and is in no other tree's maximum
    isg = ref["inv_sigma"].copy()
    isg[4, :] = 0.0
    isg[:, 4] = 0.0
    r2 = rell_wref.weighted_ref(X, nd, 1000, seed, Y=Y, inv_sigma=isg)
    got = gpu_ctx.debug_rell(X, nd, 1000, seed=seed, inv_sigma=isg)
    assert got["wkh"][4] == 1000 and got["wsh"][4] == 1000
    assert np.array_equal(got["wkh"], r2["wkh"]) and np.array_equal(got["wsh"], r2["wsh"])


def test_door_argument_checks(gpu_ctx):
    X, nd, seed, Y, ref = rell_wref.case(rell_wref.COUNT_N, 3, 1, 37)
    bad = ref["inv_sigma"].copy()
    bad[0, 1] *= 2.0                                                                    # not symmetric
    with pytest.raises(engine.PmlError) as ei:
        gpu_ctx.debug_rell(X, nd, 37, inv_sigma=bad)
    assert ei.value.code == -1
    neg = -ref["inv_sigma"]
    with pytest.raises(engine.PmlError):
        gpu_ctx.debug_rell(X, nd, 37, inv_sigma=neg)
    # a forced LDS path that cannot hold table plus matrix is refused, and the global path serves the shape
    big = rell_wref.table(5000, 64, 1)
    with pytest.raises(engine.PmlError) as ei:
        gpu_ctx.debug_rell(big, [5000], 4, path=1, weighted=True, want_y=False)
    assert ei.value.code == -1
    assert gpu_ctx.debug_rell(big, [5000], 4, weighted=True, want_y=False)["path"] == 2


def test_rell_tests_weighted(gpu_ctx):
    X, B, seed = rell_wref.table(400, 5, 31), 1000, 11
    plain = gpu_ctx.rell_tests(X, reps=B, seed=seed)
    got = gpu_ctx.rell_tests(X, reps=B, seed=seed, weighted=True)
    for f, v in plain.items():                                                          # `out`: field by field, bits included
        assert np.asarray(v).tobytes() == np.asarray(got[f]).tobytes(), f
    nd = rell_ref.default_ndraws(400)
    ref = rell_wref.weighted_ref(X, nd, B, seed)
    assert np.array_equal(got["wkh_count"], ref["wkh"]) and np.array_equal(got["wsh_count"], ref["wsh"])
    assert np.array_equal(got["wkh"], ref["wkh"] / B) and np.array_equal(got["wsh"], ref["wsh"] / B)
    assert np.array_equal(got["wkh_other"], ref["ustar"])
    nz = ref["sigma"] > 0
    assert np.array_equal(got["sigma"] > 0, nz) and np.array_equal(got["sigma"], got["sigma"].T)
    assert (np.abs(got["sigma"][nz] - ref["sigma"][nz]) / ref["sigma"][nz]).max() <= 1e-12
    # the raw ABI: a NULL weighted block is refused
    import ctypes as C
    from pepr_amd import _lib
    res = _lib.TreeTestResult()
    x = np.ascontiguousarray(X)
    assert gpu_ctx.L.pml_rell_tests_weighted(gpu_ctx.ptr, 400, 5, x.ctypes.data_as(C.POINTER(C.c_double)), None, C.byref(res), None) == -1


def _nni_neighbour(newick):
    """one NNI around the first internal edge below the root: ((A,B),C,...) -> ((A,C),B,...)"""
    kids, _, _ = util.parse_newick(newick)

    def fmt(n):
        k, name, ln = n
        return ("(" + ",".join(fmt(c) for c in k) + ")" if k else name) + ":%.10f" % ln
    i = next(j for j, c in enumerate(kids) if len(c[0]) == 2)
    inner = kids[i]
    rest = [c for j, c in enumerate(kids) if j != i]
    A, B = inner[0]
    top = [([A, rest[0]], "", inner[2]), B] + rest[1:]
    return "(" + ",".join(fmt(c) for c in top) + ");"


def test_tree_tests_weighted_end_to_end(gpu_ctx):
    """one small gene, four trees: the columns of the whole chain equal pml_rell_tests_weighted on the table it returns; the
    runConsel mirror hands back the lines of pml_catpv_table"""
    names, rows, true_nw = synth.simulate_alignment(8, 300, 77)
    gene = (names, rows)
    rnd = [synth.random_tree(8, np.random.default_rng(s), names)[0] for s in (5, 6)]
    trees = [true_nw, _nni_neighbour(true_nw), rnd[0], rnd[1]]
    B = 1000
    plain = gpu_ctx.tree_tests(gene, trees, reps=B, seed=3)
    got = gpu_ctx.tree_tests(gene, trees, reps=B, seed=3, weighted=True)
    for f, v in plain.items():
        assert np.asarray(v).tobytes() == np.asarray(got[f]).tobytes(), f
    site = got["site_lnl"]
    assert site.shape == (4, 300)
    again = gpu_ctx.rell_tests(site, reps=B, seed=3, weighted=True)
    for f in ("wkh", "wsh", "wkh_count", "wsh_count", "sigma", "wkh_other", "kh_count", "sh_count", "bp_count"):
        assert np.array_equal(got[f], again[f]), f
    ref = rell_wref.weighted_ref(site, rell_ref.default_ndraws(300), B, 3)
    print("sh", got["sh_count"], "wsh", got["wsh_count"], "reference", ref["wsh"], "kh", got["kh_count"], "wkh", got["wkh_count"], "reference", ref["wkh"],
          "margins", ref["margin_wsh"], ref["margin_wkh"], ref["margin_ustar"])
    assert np.array_equal(got["wkh_other"], ref["ustar"])
    # the mirror: weighted=True returns the catpv table with the two columns, the default is what it was
    tc = tb.TreeComparison(gpu_ctx, reps=B, seed=3, weighted=True)
    lines = tc.runConsel(tb.SequenceAlignment(names, rows), trees, "8", "PROTGAMMAWAG")
    assert lines[1].split() == "# rank item obs au np | bp pp kh sh wkh wsh |".split()
    assert lines[1:] == engine.catpv_table(tc.result) and len(lines) == 2 + len(trees)
    assert np.array_equal(tc.result["wsh_count"], got["wsh_count"])
    assert [int(l.split()[1]) for l in lines[2:]] == [1, 2, 3, 4]
    best = int(np.argmax(got["lnl"]))
    assert lines[2].split()[2] == str(best + 1) and lines[2].split()[-2] == "%.3f" % got["wsh"][best]


def test_weighted_sh_rejects_the_near_tree_more_firmly(gpu_ctx):
    """unequal variances (tests/test_tree_tests_weighted_host.py shows it with the reference alone): the best tree, a near
    neighbour (small sigma) and a far tree (large sigma).  Direction only: wsh < sh for the near tree."""
    X = rell_wref.unequal_variance_table()
    B, seed = 2000, 5
    got = gpu_ctx.rell_tests(X, reps=B, seed=seed, weighted=True)
    ref = rell_wref.weighted_ref(X, rell_ref.default_ndraws(X.shape[1]), B, seed)
    assert np.array_equal(got["wsh_count"], ref["wsh"]) and np.array_equal(got["wkh_count"], ref["wkh"])
    assert got["sigma"][0, 2] > 10 * got["sigma"][0, 1]
    assert list(got["rank"]) == [1, 2, 3]
    print("near tree: sh %.4f wsh %.4f" % (got["sh"][1], got["wsh"][1]))
    assert got["wsh"][1] < got["sh"][1]
