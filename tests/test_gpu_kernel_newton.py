"""k_newton (register form, streaming form, and the no-exchange SEQ form of both) on sumtables that the REFERENCE built, so the
kernel stands alone: f, f', f'' at a given length and the iteration's end point against tests/kref.py."""
import numpy as np
import pytest

import kh
import kref
from pepr_amd import synth

pytestmark = pytest.mark.gpu
LD = np.longdouble
# |error| / (sum_p w_p x the magnitude of the pattern terms): pinned / ceiling
TOL_F, CEIL_F = 3e-15, 1e-10            # observed 3.6e-16
TOL_PAT, CEIL_PAT = 4.6e-13, 1e-11      # observed 5.7e-14 (absolute, per-pattern lnL of magnitude up to 400)
# slices: 1, 2, 8, 63, 64 (register form); 8224 / 20000 / 100032 patterns stream
MPADS = (32, 256, 1024, 8064, 8192, 8224, 20000, 100032)


class Problem:
    """one branch: a sumtable in the tiled layout, weights with zero padding, non-zero scaling counts"""

    def __init__(self, dev, eig, rates, mpad, seed):
        rng = np.random.default_rng(seed)
        lam, U, Uinv, pi = eig
        npat = mpad - 5
        a = rng.integers(0, 20, mpad)
        b = np.where(rng.random(mpad) < 0.7, a, rng.integers(0, 20, mpad))           # related ends: the optimum is an interior length
        L = 0.01 * rng.random((4, 20, mpad)); R = 0.01 * rng.random((4, 20, mpad))
        L[:, a, np.arange(mpad)] += 1.0; R[:, b, np.arange(mpad)] += 1.0
        if seed % 2:                                                                  # unrelated ends: the optimum is the upper bound
            R = rng.random((4, 20, mpad))
        tab = np.einsum("s,si,csn->cin", pi, U, L) * np.einsum("ij,cjn->cin", Uinv, R)    # double: the table IS the input
        self.tab = tab
        self.w = rng.integers(1, 5, mpad).astype(float)
        self.w[npat:] = 0.0; self.w[5::17] = 0.0
        self.cnt = rng.integers(0, 3, mpad).astype(np.int32)
        self.mpad, self.lam, self.rates = mpad, lam, rates
        self.d_tab = dev.put(kh.clv_pack(tab.reshape(80, mpad), mpad))
        self.d_w, self.d_cnt = dev.put(self.w), dev.put(self.cnt)

    def request(self, dev, model, t0, max_iter, extras):
        r = kh.NewtonReq()
        self.out = dev.put(np.full(4, -7.0)); sync = dev.zeros(kh.NEWTON_SYNC_DOUBLES)
        r.sumtab = self.d_tab.data_ptr(); r.weight = self.d_w.data_ptr(); r.scl = self.d_cnt.data_ptr(); r.rates[:] = list(self.rates)
        r.t0 = t0; r.tol = 1e-8; r.out = self.out.data_ptr(); r.sync = sync.data_ptr(); r.md = model.data_ptr()
        r.mpad = self.mpad; r.max_iter = max_iter
        self.tdev = self.pat = None
        if extras:
            self.tdev = dev.put(np.full(2, -7.0)); self.pat = dev.put(np.full(self.mpad, -7.0))
            r.t_dev0 = self.tdev.data_ptr(); r.t_dev1 = self.tdev.data_ptr() + 8; r.patlnl = self.pat.data_ptr()
        return r

    def check(self, t_expect, what, dt=0.0):
        """out[1..3] against the reference at the returned length -> the returned length.  dt: the iteration takes its last,
        sub-tolerance step without evaluating there (newton_drive), so its sums belong to a length within dt of the returned one:
        the reference's own change over that distance is allowed on top"""
        o = self.out.cpu().numpy()
        t = float(o[0])
        if t_expect is not None:
            assert t == t_expect, (what, t, t_expect)
        lnl, d1, d2, pat = kref.newton_eval(self.tab, self.w, self.cnt, self.lam, self.rates, t)
        lr, ex = kref.newton_terms(self.lam, self.rates, t)
        tab = self.tab.astype(LD)
        f = np.einsum("cin,ci->n", tab, ex)
        a1 = np.einsum("cin,ci->n", np.abs(tab), ex * np.abs(lr)) / f
        a2 = np.einsum("cin,ci->n", np.abs(tab), ex * lr * lr) / f
        w = self.w.astype(LD)
        s0 = float((w * np.abs(pat)).sum()); s1 = float((w * a1).sum()); s2 = float((w * (a2 + a1 * a1)).sum())
        slack = (0.0, 0.0, 0.0)
        if dt:
            near = [kref.newton_eval(self.tab, self.w, self.cnt, self.lam, self.rates, t + k * dt)[:3] for k in (-1, 1)]
            slack = tuple(max(abs(float(n[i] - x)) for n in near) for i, x in enumerate((lnl, d1, d2)))
        errs = tuple(max(0.0, abs(o[i + 1] - float(x)) - slack[i]) / sc for i, (x, sc) in enumerate(((lnl, s0), (d1, s1), (d2, s2))))
        print("KERR k_newton %s mpad=%d t=%.6g  lnL %.3e  d1 %.3e  d2 %.3e (of sum w x magnitude; pinned %.1e, ceiling %.0e)"
              % (what, self.mpad, t, errs[0], errs[1], errs[2], TOL_F, CEIL_F))
        assert max(errs) <= TOL_F, ("k_newton " + what, self.mpad, t, o.tolist(), float(lnl), float(d1), float(d2))
        if self.pat is not None:
            td = self.tdev.cpu().numpy()
            assert td[0] == t and td[1] == t, ("k_newton t_dev", td, t)
            perr = float(np.abs(self.pat.cpu().numpy() - pat.astype(float)).max())
            print("KERR k_newton %s mpad=%d per-pattern lnL max error %.3e (pinned %.1e, ceiling %.0e)" % (what, self.mpad, perr, TOL_PAT, CEIL_PAT))
            assert perr <= TOL_PAT, ("k_newton patlnl " + what, self.mpad, perr)
        return t, float(d1), float(d2)


@pytest.fixture(scope="module")
def setup():
    dev = kh.Dev()
    _, _, pi3 = synth.wag_constants()
    ms, eig = kh.model_struct(pi3)
    model = dev.struct(ms)
    rates = kref.gamma_rates(0.8)
    probs = {m: Problem(dev, eig, rates, m, seed=100 + i) for i, m in enumerate(MPADS)}
    return dev, model, probs


@pytest.mark.parametrize("seq", [False, True], ids=["split", "seq"])
def test_k_newton_derivatives_at_given_lengths(setup, seq):
    """max_iter = 0: f, f', f'' at t0, register-form and streaming requests mixed in one launch in the engine's ticket order"""
    dev, model, probs = setup
    mpads = (8224, 32, 1024, 20000, 8192)
    for t0 in (1e-6, 0.01, 0.3, 5.0, 100.0):
        reqs = [probs[m].request(dev, model, t0, 0, False) for m in mpads]
        dev.newton(model, reqs, seq=seq)
        for m in mpads:
            probs[m].check(t0, "seq" if seq else "split")


def test_k_newton_iteration_end_point_and_forms_agree(setup):
    dev, model, probs = setup
    bits = {}
    for seq in (False, True):
        reqs = [probs[m].request(dev, model, 0.1, 32, True) for m in MPADS]
        dev.newton(model, reqs, seq=seq)
        for m in MPADS:
            t, d1, d2 = probs[m].check(None, "iterated " + ("seq" if seq else "split"), dt=1e-8)
            # converged by the REFERENCE's derivative (a Newton step below the tolerance), or on a bound with the gradient pointing out
            if 1e-6 < t < 34.5:
                assert d2 < 0 and abs(d1 / d2) < 1e-7, ("k_newton end point", m, t, d1, d2)
            else:
                assert (t == 34.5 and d1 > 0) or (t == 1e-6 and d1 < 0), ("k_newton bound", m, t, d1)
            both = probs[m].out.cpu().numpy().tobytes() + probs[m].pat.cpu().numpy().tobytes()
            assert bits.setdefault(m, both) == both, ("k_newton split and seq forms differ", m)
    ends = [float(probs[m].out.cpu().numpy()[0]) for m in MPADS]
    assert any(1e-6 < t < 34.5 for t in ends), ends
