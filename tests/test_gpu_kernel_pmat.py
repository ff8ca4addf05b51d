"""k_pmat and k_eigfrags driven on their own (tests/kernel_harness) against the exact P(t r) = expm(Q t r) of tests/kref.py.
Tolerances: DESIGN.md "Kernel-level error budget" (observed maximum x 8, under the ceiling a correct kernel must meet)."""
import numpy as np
import pytest

import kh
import kref
from pepr_amd import synth

pytestmark = pytest.mark.gpu

T_LIST = (0.0, 1e-9, 1e-6, 1e-3, 0.1, 1.0, 10.0, 40.0, 100.0)
ALPHAS = (0.02, 0.05, 0.8, 50.0)
# pinned (8 x observed) / ceiling, absolute.  The ceilings are NOT met (DESIGN.md "Kernel-level error budget"): observed 3.6e-15 at
# t <= 1 and 4.9e-15 over a long request list for WAG, 5.6e-15 for a +F model -- the double-precision eigensystem the kernel is
# given reproduces the identity only to that -- and on top an error that grows as |lambda_top| t r: the stationary eigenvalue
# comes out of the symmetric solver as 3e-16 instead of 0, so P(t r) carries a factor exp(lambda_top t r) (1.3e-13 at t r = 400).
TOL_P, CEIL_P = 4.5e-14, 5e-15
TOL_ROWSUM, CEIL_ROWSUM = 3e-14, 1e-14


def _drift(lam, t, rates):
    """what the not-quite-zero stationary eigenvalue of the model adds to every row of P(t r)"""
    return 1.05 * float(np.abs(lam).min()) * t * max(rates)


def _wagf_pi():
    rng = np.random.default_rng(11)
    pi = rng.random(20) + 0.2
    return pi / pi.sum()


def _expected(pi, t, rates, kind):
    """what a request's output slot stands for, as comparable arrays"""
    P = kref.p_cats(pi, t, rates)
    if kind == kh.PM_FRAGS:
        return P
    pin = np.asarray(pi, np.longdouble) / np.sum(np.asarray(pi, np.longdouble))
    if kind == kh.PM_FRAGS_PI:
        return pin[None, :, None] * P
    return np.einsum("csj,kj->cks", P, kref.indicators())          # T[c][code][s] = sum_{j in code} P_c[s][j]


def _decode(slot, kind):
    if kind == kh.PM_TIPTABLE:
        t, pad = kh.tiptab_unpack(slot)
        assert np.all(pad == 0.0)
        return t
    assert np.all(slot[kh.PFRAG:] == 7.0)            # a fragment set is PFRAG doubles of its FRAG_STRIDE slot: the rest is untouched
    return kh.frag_unpack(slot)


def _req(t, rates, kind, tp=None, md=None):
    r = kh.PmatReq()
    r.t = t; r.rates[:] = list(rates); r.kind = kind; r.pad = 0
    r.tp = tp; r.md = md
    return r


def test_k_pmat_against_expm_over_lengths_and_rates():
    dev = kh.Dev()
    _, _, pi3 = synth.wag_constants()
    ms, (lam, _, _, _) = kh.model_struct(pi3)
    model = dev.struct(ms)
    rate_sets = [kref.gamma_rates(a) for a in ALPHAS] + [(1.0, 1.0, 1.0, 1.0)]
    cases = [(t, rs, kind) for t in T_LIST for rs in rate_sets for kind in (kh.PM_FRAGS, kh.PM_FRAGS_PI, kh.PM_TIPTABLE)]
    out = dev.pmat([_req(t, rs, kind) for t, rs, kind in cases], model)
    worst = {}
    for (t, rs, kind), slot in zip(cases, out):
        got, ref = _decode(slot, kind), _expected(pi3, t, rs, kind)
        assert np.all(got >= 0.0)
        err = max(0.0, float(np.abs(got - ref).max()) - _drift(lam, t, rs))
        if kind == kh.PM_FRAGS:
            rs_err = float(np.abs(got.astype(np.longdouble).sum(2) - 1).max())
        elif kind == kh.PM_TIPTABLE:
            rs_err = float(np.abs(got[:, 22, :].astype(np.longdouble) - 1).max())        # code 22 = every state: a row sum of P
        else:
            rs_err = 0.0
        rs_err = max(0.0, rs_err - _drift(lam, t, rs))
        key = "t=%g" % t
        w = worst.get(key, (0.0, 0.0))
        worst[key] = (max(w[0], err), max(w[1], rs_err))
    for k, (e, r) in worst.items():
        print("KERR k_pmat %-8s (less lambda_top t r) max |P - expm| %.3e (pinned %.1e, ceiling %.0e)  max |row sum - 1| %.3e (pinned %.1e, ceiling %.0e)"
              % (k, e, TOL_P, CEIL_P, r, TOL_ROWSUM, CEIL_ROWSUM))
    for k, (e, r) in worst.items():
        assert e <= TOL_P, ("k_pmat entry", k, e)
        assert r <= TOL_ROWSUM, ("k_pmat row sum", k, r)


@pytest.mark.parametrize("n", [1, 3, 4, 5, 2047, 2048, 2049])
def test_k_pmat_request_counts_and_device_lengths(n):
    """the persistent waves wrap around 512 workgroups x 4 waves; every other request reads its length from device memory (tp)
    while its `t` holds garbage; kinds are mixed in one list"""
    dev = kh.Dev()
    _, _, pi3 = synth.wag_constants()
    ms, _ = kh.model_struct(pi3)
    model = dev.struct(ms)
    rates = kref.gamma_rates(0.8)
    pool = [0.013, 0.05, 0.11, 0.27, 0.5, 0.9, 1.7, 3.1]
    lens = dev.put(np.array(pool))
    want = {(k, kind): _expected(pi3, pool[k], rates, kind) for k in range(len(pool)) for kind in range(3)}
    reqs, keys = [], []
    for i in range(n):
        k, kind = (i * 5 + 3) % len(pool), i % 3
        if i % 2:
            reqs.append(_req(float("nan") if i % 4 == 1 else 1e300, rates, kind, tp=lens.data_ptr() + 8 * k))
        else:
            reqs.append(_req(pool[k], rates, kind))
        keys.append((k, kind))
    out = dev.pmat(reqs, model)
    err = max(float(np.abs(_decode(slot, key[1]) - want[key]).max()) for key, slot in zip(keys, out))
    print("KERR k_pmat n=%d max error %.3e (pinned %.1e)" % (n, err, TOL_P))
    assert err <= TOL_P, ("k_pmat request list", n, err)


def test_k_pmat_per_request_models():
    dev = kh.Dev()
    _, _, pi3 = synth.wag_constants()
    pis = [pi3, _wagf_pi()]
    structs = [kh.model_struct(p)[0] for p in pis]
    models = dev.put(np.frombuffer(b"".join(bytes(s) for s in structs), np.uint8).copy())
    size = len(bytes(structs[0]))
    rates = kref.gamma_rates(0.5)
    cases = [(i % 2, t, kind) for i, (t, kind) in enumerate((t, kind) for t in (1e-6, 0.2, 2.0) for kind in range(3))]
    cases += [(1 - m, t, kind) for m, t, kind in cases]
    out = dev.pmat([_req(t, rates, kind, md=models.data_ptr() + m * size) for m, t, kind in cases], None, per_request=True)
    err = max(float(np.abs(_decode(slot, kind) - _expected(pis[m], t, rates, kind)).max()) for (m, t, kind), slot in zip(cases, out))
    print("KERR k_pmat per-request models max error %.3e (pinned %.1e)" % (err, TOL_P))
    assert err <= TOL_P, ("k_pmat per-request model", err)


@pytest.mark.parametrize("n", [1, 3])
def test_k_eigfrags_sets_follow_their_definitions(n):
    dev = kh.Dev()
    _, _, pi3 = synth.wag_constants()
    rng = np.random.default_rng(4)
    pis = [pi3] + [rng.random(20) + 0.1 for _ in range(n - 1)]
    built = [kh.model_struct(p) for p in pis]
    models = dev.put(np.frombuffer(b"".join(bytes(s) for s, _ in built), np.uint8).copy())
    out = dev.eigfrags(models, n).cpu().numpy().reshape(n, 2, kh.PFRAG)
    for g, (_, (lam, U, Uinv, pi)) in enumerate(built):
        s0, s1 = kh.frag_unpack(out[g, 0]), kh.frag_unpack(out[g, 1])
        # set 0: x_i = sum_s pi_s U[s][i] A[s] -> M[i][s] = pi_s U[s][i]; set 1: y_i = sum_j Uinv[i][j] B[j] -> M = Uinv; all four categories
        for c in range(4):
            assert np.array_equal(s0[c], (pi[:, None] * U).T), ("k_eigfrags set 0", g, c)
            assert np.array_equal(s1[c], Uinv), ("k_eigfrags set 1", g, c)


def test_harness_refuses_what_the_engine_never_sends():
    """a mistake in a test is an exception before the launch: short output, bad kind, pointer outside the listed tensors"""
    dev = kh.Dev()
    _, _, pi3 = synth.wag_constants()
    model = dev.struct(kh.model_struct(pi3)[0])
    rates = (1.0, 1.0, 1.0, 1.0)
    with pytest.raises(kh.KhError):
        dev.pmat([_req(0.1, rates, 3)], model)
    with pytest.raises(kh.KhError):
        dev.pmat([_req(0.1, rates, 0, tp=model.data_ptr() + (1 << 30))], model)
    with pytest.raises(kh.KhError):
        dev.pmat([_req(0.1, rates, 0)], None, per_request=True)
    stab = dev.zeros(kh.clv_doubles(64))
    r = kh.NewtonReq()
    r.sumtab = stab.data_ptr(); r.mpad = 96               # a table of one tile and vectors of 96 entries ...
    r.weight = dev.zeros(96).data_ptr(); r.scl = dev.zeros(96, np.int32).data_ptr(); r.out = dev.zeros(4).data_ptr()
    r.sync = dev.zeros(kh.NEWTON_SYNC_DOUBLES).data_ptr(); r.md = model.data_ptr(); r.tol = 1e-8; r.t0 = 0.1
    r.rates[:] = rates
    with pytest.raises(kh.KhError):
        r.mpad = 160                                      # ... offered as 160 patterns
        dev.newton(model, [r])
    with pytest.raises(kh.KhError):
        r.mpad = 40                                       # no multiple of 32
        dev.newton(model, [r])
