"""Tree selection tests, the parts that need no GPU: the host AU fit (pml_au_fit) against the numpy / scipy restatement in
tests/rell_ref.py, argument checks of the device entry points, the runConsel mirror's model check, and the reference's own
two formulations of the sequential sum."""
import ctypes as C

import numpy as np
import pytest

import rell_ref
from pepr_amd import _lib, engine, tree_builder as tb

R10 = np.arange(5, 15) / 10.0
# bootstrap counts of one tree at the ten scales (B replicates each), recorded from rell_ref.tests on the synthetic table of
# rell_ref.synthetic_table() (B = 2000, seed 11) and edge cases written by hand
RECORDED = {
    "best":            (2000, [1769, 1861, 1867, 1902, 1931, 1943, 1954, 1961, 1971, 1978]),
    "near_tie":        (2000, [193, 121, 117, 89, 56, 53, 45, 38, 29, 21]),
    "a_scale_at_0":    (2000, [38, 18, 16, 9, 13, 4, 1, 1, 0, 1]),                       # dropped: 9 usable
    "a_scale_at_B":    (2000, [2000, 1990, 1985, 1980, 1970, 1960, 1950, 1940, 1930, 1920]),
    "one_usable":      (2000, [0, 0, 0, 0, 0, 3, 0, 0, 0, 0]),                           # -> count[k1] / B
    "all_zero":        (2000, [0] * 10),
    "all_B":           (2000, [2000] * 10),
    "two_usable":      (2000, [0, 0, 0, 0, 5, 9, 0, 0, 0, 0]),
    "middling":        (2000, [900, 950, 1000, 1020, 1040, 1060, 1075, 1090, 1100, 1110]),
    "b10":             (100000, [91234, 92011, 92500, 93000, 93321, 93600, 93900, 94100, 94300, 94500]),
}
# Both sides do double arithmetic on identical integers: the ceiling is 1e-9.  Observed maximum of |dAU|, |dd|, |dc| over the
# vectors above: 3.5e-14 (the exactly determined two-scale fit); pinned at about 8x that, the project's convention.
AU_TOL = 3e-13


def test_au_fit_matches_reference():
    worst = 0.0
    for name, (B, cnt) in RECORDED.items():
        a, b = engine.au_fit(R10, cnt, B), rell_ref.au_fit(R10, cnt, B)
        d = max(abs(a[k] - b[k]) for k in ("au", "d", "c"))
        worst = max(worst, d)
        print("%-14s AU %.15g ref %.15g  max|d| %.3g  nused %d" % (name, a["au"], b["au"], d, a["nused"]))
        assert a["nused"] == b["nused"], name
        assert d <= AU_TOL, (name, a, b)
        assert abs(a["rss"] - b["rss"]) <= 1e-9 * max(1.0, abs(b["rss"])), (name, a, b)
    print("observed maximum", worst)
    assert worst <= AU_TOL < 1e-9


def test_au_fit_edge_cases():
    B = 2000
    assert engine.au_fit(R10, RECORDED["a_scale_at_0"][1], B)["nused"] == 9
    assert engine.au_fit(R10, RECORDED["a_scale_at_B"][1], B)["nused"] == 9
    one = engine.au_fit(R10, RECORDED["one_usable"][1], B)
    assert one == {"au": 3 / 2000, "d": 0.0, "c": 0.0, "rss": 0.0, "nused": 1}           # k1 = the scale 1.0 (index 5)
    zero = engine.au_fit(R10, RECORDED["all_zero"][1], B)
    assert zero["au"] == 0.0 and zero["nused"] == 0
    assert engine.au_fit(R10, RECORDED["all_B"][1], B)["au"] == 1.0
    # the fallback scale is the one closest to 1, the first of equals -- whatever the order of the scales
    r = np.array([1.4, 0.9, 1.1, 0.5])
    assert engine.au_fit(r, [0, 7, 9, 0], 100)["nused"] == 2
    assert engine.au_fit(r, [0, 7, 0, 0], 100)["au"] == 0.07
    assert engine.au_fit(r, [0, 0, 9, 0], 100)["au"] == 0.0
    # usable scales that do not determine the two parameters (one r): no fit, and nused says so
    same = engine.au_fit([1.0, 1.0, 1.0], [30, 40, 50], 100)
    assert same == {"au": 0.3, "d": 0.0, "c": 0.0, "rss": 0.0, "nused": 1}


def test_au_fit_argument_checks():
    L = _lib.load()
    r = (C.c_double * 2)(0.5, 1.0)
    cnt = (C.c_longlong * 2)(1, 2)
    au = C.c_double()
    assert L.pml_au_fit(2, r, cnt, 10, C.byref(au), None, None, None, None) == 0        # the optional outputs may be NULL
    assert L.pml_au_fit(0, r, cnt, 10, C.byref(au), None, None, None, None) == -1
    assert L.pml_au_fit(2, None, cnt, 10, C.byref(au), None, None, None, None) == -1
    assert L.pml_au_fit(2, r, None, 10, C.byref(au), None, None, None, None) == -1
    assert L.pml_au_fit(2, r, cnt, 0, C.byref(au), None, None, None, None) == -1
    assert L.pml_au_fit(2, r, cnt, 10, None, None, None, None, None) == -1
    cnt[1] = 11
    assert L.pml_au_fit(2, r, cnt, 10, C.byref(au), None, None, None, None) == -1       # a count above B
    cnt[1] = 2; r[0] = 0.0
    assert L.pml_au_fit(2, r, cnt, 10, C.byref(au), None, None, None, None) == -1       # a scale must be positive


def test_device_entry_points_refuse_a_null_context():
    """All this side of the suite can show without a device: a NULL context is PML_EINVAL and nothing is dereferenced, and the
    free function takes NULL and an empty result.  The shape checks (T = 1, T = 65, N >= 2^31) and the NULL pointers are
    exercised with a live context in tests/test_gpu_tree_tests.py::test_argument_checks_with_a_context."""
    L = _lib.load()
    x = np.zeros(8)
    res = _lib.TreeTestResult()
    xp = x.ctypes.data_as(C.POINTER(C.c_double))
    nd = (C.c_longlong * 1)(4)
    assert L.pml_rell_tests(None, 4, 2, xp, None, C.byref(res)) == -1
    assert L.pml_tree_tests(None, None, 2, None, None, None, None, C.byref(res), None) == -1
    assert L.pml_debug_rell(None, 4, 2, xp, 1, nd, 1, 0, 0, None, None, None, None, None, None) == -1
    L.pml_tree_test_result_free(None)                                                   # harmless
    L.pml_tree_test_result_free(C.byref(res))
    assert res.ntrees == 0 and not res.au


def test_mirror_refuses_unbuilt_model_before_any_device():
    aln = tb.SequenceAlignment(["a", "b", "c", "d"], ["AR", "AR", "AQ", "AQ"])
    trees = ["((a,b),c,d);", "((a,c),b,d);"]
    for name in ("PROTGAMMALGF", "PROTCATWAG", "GTRGAMMA"):
        with pytest.raises(ValueError):
            tb.TreeComparison().runConsel(aln, trees, "8", name)                       # no context was ever created


def test_reference_sequential_sum_formulations_agree():
    """rell_ref adds draw j of every replicate before draw j + 1; np.cumsum along the draws is the same chain of roundings.
    np.sum (pairwise) is not: the check would be vacuous if the three agreed."""
    rng = np.random.default_rng(5)
    X = -rng.gamma(2.0, 1.5, size=(5, 400))
    nd = [200, 560]
    a = rell_ref.replicate_sums(X, nd, 64, 3)
    b = rell_ref.replicate_sums(X, nd, 64, 3, use_cumsum=True)
    assert np.array_equal(a, b)
    s = rell_ref.draws(3, 1, 64, np.arange(64), 560, 400)
    pairwise = np.ascontiguousarray(X.T[s].transpose(0, 2, 1)).sum(axis=2)          # contiguous axis: numpy adds pairwise
    assert np.allclose(pairwise, a[1], rtol=1e-12) and not np.array_equal(pairwise, a[1])
    assert s.min() >= 0 and s.max() < 400


def test_reference_meaning_on_the_synthetic_table():
    """the conditions the GPU suite asks of the device hold for the reference alone"""
    X = rell_ref.synthetic_table()
    B = 2000
    r = rell_ref.tests(X, B, 11)
    assert r["k1"] == 5
    assert r["sh_count"][0] == B and r["kh_count"][0] == B
    assert np.all(r["bp_count"][:, 3] == 0) and r["sh_count"][3] == B and r["kh_count"][3] == B     # the duplicate: ties go to the lowest index
    assert np.all(r["bp_count"][:, 4] == 0) and r["sh_count"][4] == 0 and r["kh_count"][4] == 0 and r["au"][4] == 0.0
    assert np.all(r["bp_count"].sum(axis=1) == B)
    assert r["fits"][0]["nused"] == 10 and r["fits"][1]["nused"] == 10
    assert r["au"][0] > 0.9 and 0.005 < r["au"][1] < 0.2 and r["au"][2] < r["au"][1]
