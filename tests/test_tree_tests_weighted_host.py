"""Weighted tree selection tests (wKH, wSH), the parts that need no GPU: pml_catpv_table against literal lines, the NULL-context
refusals of the new device entry points, the reference's own properties, and the MARGIN CHECK that licenses the exact-equality
assertions of tests/test_gpu_tree_tests_weighted.py: for every (seed, shape) the GPU tests use, no comparison the reference
makes is within 1e-9 (relative) of a tie, so an implementation's free summation order in sigma (a few 1e-16) cannot flip one."""
import ctypes as C

import numpy as np
import pytest

import rell_ref
import rell_wref
from pepr_amd import _lib, engine

MARGIN = 1e-9


def _hand_made():
    """four trees; trees 1 and 2 share rank 2 (the table takes ranks as given: equal ranks in index order); tree 3 has rank 104"""
    return {"ntrees": 4, "rank": [1, 2, 2, 104], "obs": [-3.24, 3.24, 12.04, 1234.56], "au": [0.8768, 0.2343, 0.0496, 0.0],
            "np": [0.7, 0.2, 0.1, 0.0], "bp": [0.7004, 0.2, 0.0996, 0.0], "pp": [0.9, 0.09, 0.01, 1e-30], "kh": [0.61, 0.39, 0.05, 0.0],
            "sh": [1.0, 0.5, 0.1251, 0.0006]}


def test_catpv_table_literal_lines():
    r = _hand_made()
    w = {"wkh": [0.6, 0.38, 0.0494, 0.0], "wsh": [0.999, 0.4123, 0.1, 1.0]}
    assert engine.catpv_table(r, w) == [
        "# rank item      obs     au     np |     bp     pp     kh     sh    wkh    wsh |",
        "#    1    1     -3.2  0.877  0.700 |  0.700  0.900  0.610  1.000  0.600  0.999 |",
        "#    2    2      3.2  0.234  0.200 |  0.200  0.090  0.390  0.500  0.380  0.412 |",
        "#    2    3     12.0  0.050  0.100 |  0.100  0.010  0.050  0.125  0.049  0.100 |",
        "#  104    4   1234.6  0.000  0.000 |  0.000  0.000  0.000  0.001  0.000  1.000 |",
    ]
    # no weighted columns: "-" in both
    assert engine.catpv_table(r) == [
        "# rank item      obs     au     np |     bp     pp     kh     sh    wkh    wsh |",
        "#    1    1     -3.2  0.877  0.700 |  0.700  0.900  0.610  1.000      -      - |",
        "#    2    2      3.2  0.234  0.200 |  0.200  0.090  0.390  0.500      -      - |",
        "#    2    3     12.0  0.050  0.100 |  0.100  0.010  0.050  0.125      -      - |",
        "#  104    4   1234.6  0.000  0.000 |  0.000  0.000  0.000  0.001      -      - |",
    ]
    # rows follow the rank, whatever the order of the trees; a result dict that carries wkh / wsh is printed with them
    r2 = dict(r, rank=[3, 1, 2, 4], **w)
    lines = engine.catpv_table(r2)
    assert [l.split()[1:3] for l in lines[1:]] == [["1", "2"], ["2", "3"], ["3", "1"], ["4", "4"]]
    assert lines[1].endswith(" 0.380  0.412 |")


def test_catpv_table_argument_checks():
    L = _lib.load()
    out = C.c_void_p()
    res, w = _lib.TreeTestResult(), _lib.TreeTestWeighted()
    assert L.pml_catpv_table(None, None, C.byref(out)) == -1
    assert L.pml_catpv_table(C.byref(res), None, None) == -1
    assert L.pml_catpv_table(C.byref(res), None, C.byref(out)) == -1 and not out.value          # an empty result
    with pytest.raises(ValueError):
        engine.catpv_table(_hand_made(), {"wkh": [0.1], "wsh": [0.1]})
    # a weighted block of another tree count
    r = _hand_made()
    keep = [np.array(r[f], dtype=np.float64) for f in ("obs", "au", "np", "bp", "pp", "kh", "sh")]
    rank = np.array(r["rank"], dtype=np.int32)
    res.ntrees, res.rank = 4, rank.ctypes.data_as(C.POINTER(C.c_int))
    for f, a in zip(("obs", "au", "np", "bp", "pp", "kh", "sh"), keep):
        setattr(res, f, a.ctypes.data_as(C.POINTER(C.c_double)))
    two = np.zeros(4)
    w.ntrees, w.wkh, w.wsh = 3, two.ctypes.data_as(C.POINTER(C.c_double)), two.ctypes.data_as(C.POINTER(C.c_double))
    assert L.pml_catpv_table(C.byref(res), C.byref(w), C.byref(out)) == -1
    w.ntrees = 4
    assert L.pml_catpv_table(C.byref(res), C.byref(w), C.byref(out)) == 0
    L.pml_free(out)


def test_weighted_entry_points_refuse_a_null_context():
    L = _lib.load()
    x = np.zeros(8)
    xp = x.ctypes.data_as(C.POINTER(C.c_double))
    res, w = _lib.TreeTestResult(), _lib.TreeTestWeighted()
    nd = (C.c_longlong * 1)(4)
    cnt = np.zeros(8, dtype=np.int64)
    lp = cnt.ctypes.data_as(C.POINTER(C.c_longlong))
    assert L.pml_rell_tests_weighted(None, 4, 2, xp, None, C.byref(res), C.byref(w)) == -1
    assert L.pml_tree_tests_weighted(None, None, 2, None, None, None, None, C.byref(res), C.byref(w), None) == -1
    assert L.pml_debug_rell_weighted(None, 4, 2, xp, 1, nd, 1, 0, 0, None, lp, lp, lp, None, None, None, None, lp, lp) == -1
    assert res.ntrees == 0 and w.ntrees == 0 and not w.wkh
    L.pml_tree_test_weighted_free(None)                                                 # harmless
    L.pml_tree_test_weighted_free(C.byref(w))
    assert w.ntrees == 0 and not w.sigma


@pytest.mark.parametrize("N,T,K,B", rell_wref.all_count_cases())
def test_margins_of_every_gpu_case(N, T, K, B):
    """no comparison of the reference is closer than 1e-9 (relative) to a tie; if one is, choose another seed in rell_wref.case_seed"""
    ref = rell_wref.case(N, T, K, B)[4]
    print("N %d T %d K %d B %d: margins wsh %.3g wkh %.3g u* %.3g" % (N, T, K, B, ref["margin_wsh"], ref["margin_wkh"], ref["margin_ustar"]))
    assert ref["margin_wsh"] >= MARGIN and ref["margin_wkh"] >= MARGIN and ref["margin_ustar"] >= MARGIN


def test_margins_of_the_other_gpu_tables():
    """the tables of the GPU tests that go through pml_rell_tests_weighted (default ladder)"""
    for X, B, seed in ((rell_wref.table(400, 5, 31), 1000, 11), (rell_wref.unequal_variance_table(), 2000, 5)):
        nd = rell_ref.default_ndraws(X.shape[1])
        ref = rell_wref.weighted_ref(X, nd, B, seed)
        assert min(ref["margin_wsh"], ref["margin_wkh"], ref["margin_ustar"]) >= MARGIN


def test_reference_sigma_two_ways():
    """the longdouble two-pass sigma against the textbook var(d) of numpy (ddof = 1) times N; zeros where defined"""
    X = rell_wref.table(200, 5, 9)
    sig = rell_wref.pair_sigma(X)
    assert np.array_equal(sig, sig.T) and np.all(np.diag(sig) == 0) and sig[0, 3] == 0.0
    for u, t in ((0, 1), (1, 4), (2, 3)):
        d = X[u] - X[t]
        assert abs(sig[u, t] - np.sqrt(200 * d.var(ddof=1))) <= 1e-12 * sig[u, t]
    assert not rell_wref.pair_sigma(X[:, :1]).any()                                      # N = 1
    inv = rell_wref.inv_of(sig)
    assert inv[0, 3] == 0.0 and inv[1, 2] == 1.0 / sig[1, 2]


def test_reference_degenerate_and_single_pair():
    # N = 1: no pair anywhere, every weighted p-value is 1
    N, T, K, B = 1, 5, 1, 37
    ref = rell_wref.case(N, T, K, B)[4]
    assert np.all(ref["wkh"] == B) and np.all(ref["wsh"] == B) and np.all(ref["ustar"] == -1)
    # a duplicate is excluded from its pair only: tree 0 and tree 3 still have the other three
    X, nd, seed, Y, ref = rell_wref.case(200, 5, 1, 1000)
    assert ref["sigma"][0, 3] == 0.0 and ref["ustar"][0] not in (-1, 3) and ref["ustar"][3] not in (-1, 0)
    assert np.array_equal(ref["wsh"][[0]], ref["wsh"][[3]]) and np.array_equal(ref["wkh"][[0]], ref["wkh"][[3]])
    # T = 2: a single pair, the sigma cancels: wkh = wsh = kh
    X, nd, seed, Y, ref = rell_wref.case(200, 2, 10, 1000)
    _, kh, _, _ = rell_ref.counts(X, nd, 1000, seed, Y=Y)
    assert np.array_equal(ref["wkh"], kh) and np.array_equal(ref["wsh"], kh)


def test_reference_weighted_sh_is_less_conservative_for_the_near_tree():
    """unequal variances: the far tree's spread inflates max_u C_u, so plain SH cannot reject the near neighbour as firmly as the
    weighted form, which measures every competitor in units of its own sigma.  Direction only."""
    X = rell_wref.unequal_variance_table()
    B, seed = 2000, 5
    nd = rell_ref.default_ndraws(X.shape[1])
    Y = rell_ref.replicate_sums(X, nd, B, seed)
    _, kh, sh, _ = rell_ref.counts(X, nd, B, seed, Y=Y)
    ref = rell_wref.weighted_ref(X, nd, B, seed, Y=Y)
    print("sigma", ref["sigma"], "sh", sh, "wsh", ref["wsh"], "kh", kh, "wkh", ref["wkh"])
    assert ref["sigma"][0, 2] > 10 * ref["sigma"][0, 1]
    assert ref["wsh"][1] < sh[1]
    assert ref["L"][0] > ref["L"][1] > ref["L"][2]                                      # best, near, far
