"""CPU checks of the kernel-test layer: the ctypes mirrors of tests/kh.py against the structs the harness was compiled with
(layout drift fails here, before anything is launched), the packers against each other, and the references of tests/kref.py
against three independent values."""
import ctypes as C
import os

import numpy as np
import pytest

import kh
import kref
from pepr_amd import synth
from util import numpy_lnl

pytestmark = pytest.mark.skipif(not os.path.exists(kh.LIB_PATH), reason="tests/kernel_harness/libkh.so not built (build())")
LD = np.longdouble


def test_struct_layouts_match_the_compiled_header():
    L = kh.lib()
    for name, cls in kh.MIRRORS.items():
        assert C.sizeof(cls) == L.kh_sizeof(name.encode()), name
        for field, _ in cls._fields_:
            assert getattr(cls, field).offset == L.kh_offsetof(name.encode(), field.encode()), (name, field)
    assert L.kh_sizeof(b"NoSuchStruct") == -1 and L.kh_offsetof(b"NvOp", b"nosuch") == -1
    for k, v in kh.CONSTANTS.items():
        assert L.kh_const(k.encode()) == v, k


def test_layout_functions_match_the_compiled_header():
    L = kh.lib()
    for mpad in (32, 64, 96, 128, 160, 256, 4128, 8192, 8224, 20000, 100032):
        assert kh.clv_doubles(mpad) == L.kh_clv_doubles(mpad)
        assert kh.newton_split(mpad) == L.kh_newton_split(mpad) and kh.newton_slice(mpad) == L.kh_newton_slice(mpad)
        assert kh.newton_reg_form(mpad) == bool(L.kh_newton_reg_form(mpad))
        # the slices cover the request
        assert kh.newton_split(mpad) * kh.newton_slice(mpad) >= mpad
    for row, p in ((0, 0), (79, 127), (3, 128), (41, 4127)):
        assert kh.clv_index(row, p) == L.kh_clv_index(row, p)


def test_packers_round_trip():
    rng = np.random.default_rng(1)
    a = rng.random((80, 150))
    flat = kh.clv_pack(a, 160)
    assert flat.size == kh.clv_doubles(160) and np.array_equal(kh.clv_unpack(flat, 160)[:, :150], a)
    assert flat[kh.clv_index(7, 131)] == a[7, 131]
    m = rng.random((4, 20, 20))
    f = kh.frag_pack(m)
    assert np.array_equal(kh.frag_unpack(f), m)
    # kernels.hip frag_decode: element 4k+i of fragment (c, st, kk) = M_c[4 st + i][4 kk + k]
    c, st, kk, k, i = 2, 3, 1, 2, 3
    assert f[((c * 25 + st * 5 + kk) << 4) + 4 * k + i] == m[c, 4 * st + i, 4 * kk + k]
    t = rng.random((4, 23, 20))
    tt = kh.tiptab_pack(t)
    assert tt.size == kh.TIPTAB_DOUBLES and np.array_equal(kh.tiptab_unpack(tt)[0], t)
    assert tt[((1 * 23 + 22) * 4 + 3) * 6 + 2] == t[1, 22, 4 * 2 + 3]           # T[c][code][q][kk], s = 4 kk + q
    # ticket table: register-form requests first, ticket0 relative to the request's kernel
    tk, t0, nreg, nstream = kh.newton_tickets([256, 8224, 32])
    assert tk == [0, 0, 2] + [1] * 64 and t0 == [0, 0, 2] and (nreg, nstream) == (3, 64)


def test_exact_p_against_scipy_expm():
    from scipy.linalg import expm
    _, pi, pi3 = synth.wag_constants()
    for p in (pi, pi3):
        Q = synth.wag_q(np.asarray(p, float))
        for t in (0.0, 1e-6, 1e-3, 0.1, 1.0, 10.0):
            P = kref.p_exact(p, t, 1.0)
            assert np.abs(P.astype(float) - expm(Q * t)).max() < 2e-14, t
            assert np.abs(P.sum(1) - 1).max() < 1e-18 and P.min() > -1e-40
    # the bulk form (50-digit spectral) is the definition (mpmath.expm) to longdouble rounding, at the branch floor, at the rate of
    # the slowest category of alpha = 0.02 and at saturation alike
    for tr in (0.0, 4.4e-31 * 1e-6, 1e-9, 1e-6, 0.37, 100.0 * 3.9):
        A, B = kref.p_exact(pi3, tr, 1.0), kref.p_expm(pi3, tr, 1.0)
        assert np.abs(A - B).max() < 3e-19, tr
    # the rate matrix has one expected substitution per unit time
    Qm, pim = kref.q_mp(pi)
    assert abs(float(sum(pim[i] * Qm[i, i] for i in range(20))) + 1.0) < 1e-15


def test_gamma_rates_against_scipy():
    for alpha in (0.02, 0.05, 0.8, 50.0):
        r = np.array(kref.gamma_rates(alpha))
        assert abs(r.mean() - 1.0) < 1e-15 and np.all(np.diff(r) > 0)
        s = synth.gamma_mean_rates(alpha, 4)
        assert np.allclose(r[1:], s[1:], rtol=1e-9, atol=0), (alpha, r, s)
        assert abs(r[0] - s[0]) < 1e-12          # the slowest rate at alpha = 0.02 is ~1e-47: absolute


def test_composed_newviews_give_numpy_lnl():
    """((A,B),(C,D),E) by kref newviews / cherry / evaluate on the exact P against util.numpy_lnl (eigensystem P, log-space scaling)"""
    names, rows, _ = synth.simulate_alignment(5, 60, 3, missing_frac=0.2)
    code = {c: i for i, c in enumerate(synth.AA)}
    codes = {n: np.array([code.get(ch, 20 if ch == "B" else 21 if ch == "Z" else 22) for ch in r.upper()]) for n, r in zip(names, rows)}
    a, b, c, d, e = names
    nw = "((%s:0.11,%s:0.23):0.07,(%s:0.05,%s:0.4):0.31,%s:0.13);" % (a, b, c, d, e)
    _, _, pi3 = synth.wag_constants()
    alpha = 0.6
    rates = kref.gamma_rates(alpha)
    P = lambda t: kref.p_cats(pi3, t, rates)                       # noqa: E731
    x = kref.cherry_operand(P(0.11), codes[a], P(0.23), codes[b])    # CLV at (A,B)
    y = kref.newview(P(0.05), kref.tip_operand(codes[c]), P(0.4), kref.tip_operand(codes[d]))
    top = kref.newview(P(0.07), x, P(0.31), y)                       # the root's CLV seen from E
    site = kref.evaluate(pi3, P(0.13), kref.tip_operand(codes[e]), top)
    tot, per = numpy_lnl(names, rows, nw, alpha)
    assert np.abs(site.astype(float) - per).max() < 1e-10
    assert abs(float(site.sum()) - tot) < 1e-9
    # the same through the sumtable of the edge to E: f(t) of Newton's form reproduces the per-pattern lnL
    _, eig = kh.model_struct(pi3)
    tab = kref.sumtable(eig, kref.tip_operand(codes[e]), top)
    w = np.ones(60)
    lnl, _, _, pat = kref.newton_eval(tab, w, np.zeros(60), eig[0], rates, 0.13)
    assert np.abs((pat - site).astype(float)).max() < 1e-10 and abs(float(lnl) - tot) < 1e-9


def test_newton_reference_derivatives_by_finite_difference():
    rng = np.random.default_rng(5)
    _, _, pi3 = synth.wag_constants()
    _, eig = kh.model_struct(pi3)
    rates = kref.gamma_rates(0.8)
    n = 40
    L = rng.random((4, 20, n)); R = rng.random((4, 20, n))
    tab = kref.sumtable(eig, L, R)
    w = rng.integers(0, 4, n).astype(float)
    cnt = rng.integers(0, 3, n)
    for t in (0.01, 0.3, 5.0):
        hh = LD(2.0) ** int(np.round(np.log2(1e-5 * max(t, 0.1))))     # a power of two: t - h and t + h are exact doubles
        f = [kref.newton_eval(tab, w, cnt, eig[0], rates, t + k * float(hh)) for k in (-1, 0, 1)]
        d1 = (f[2][0] - f[0][0]) / (2 * hh)
        d2 = (f[2][1] - f[0][1]) / (2 * hh)          # f'' against the difference of f' (a second difference of lnL drowns in its rounding)
        assert abs(d1 - f[1][1]) < 1e-6 * max(1, abs(f[1][1])), (t, d1, f[1][1])
        assert abs(d2 - f[1][2]) < 1e-6 * max(1, abs(f[1][2])), (t, d2, f[1][2])


def test_definitions_of_the_small_kernels():
    # the counter hash: fixed values of the published splitmix64 finaliser
    assert kref.mix64(0) == 0 and kref.mix64(1) == 0x5692161D100B05E5
    cols = kref.sh_columns(7, 3, 101)
    assert len(cols) == 101 and all(0 <= c < 101 for c in cols)
    # Gamma20: all traversals at the same count -> plain mixture, count applied once
    rng = np.random.default_rng(2)
    tab = rng.random((20, 6)); w = rng.random(20)
    wt = np.array([1, 2, 0, 1, 3, 1.0])
    lnl, pat = kref.g20(tab, np.full((5, 6), 2), wt, w)
    ref = np.log((w[:, None] * tab).sum(0)) - 2 * kh.LOG_2_256
    assert np.abs(pat.astype(float)[wt != 0] - ref[wt != 0]).max() < 1e-12 and pat[2] == 0
    assert abs(float(lnl) - (wt * ref).sum()) < 1e-10
