"""Models beyond WAG on the device: registered rate matrices (own and empirical frequencies), per-gene matrices in resident
batches, the batched model-build kernel (k_model), PROTGAMMAGTR, pml_model_eval and the raxmlHPC shim's -m resolution.
Parity is against oracle/ with a po._ModelStruct filled from numpy's eigh for the same matrix."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from pepr_amd import engine, synth
from util import rf_collapsed
from test_models_host import paml_text

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RX = os.path.join(ROOT, "bin", "raxmlHPC")
EPS_GTR = 0.01


def random_matrix(seed):
    rng = np.random.default_rng(seed)
    ex = np.exp(rng.normal(0.0, 1.0, 190))
    pi = np.maximum(rng.dirichlet(np.full(20, 5.0)), 0.005)
    return ex, pi / pi.sum()


def build_q(ex, pi, dtype=np.float64):
    S = np.zeros((20, 20), dtype=dtype)
    k = 0
    for i in range(1, 20):
        for j in range(i):
            S[i, j] = S[j, i] = ex[k]
            k += 1
    pi = np.asarray(pi, dtype=dtype)
    pi = pi / pi.sum()
    Q = S * pi[None, :]
    np.fill_diagonal(Q, -Q.sum(1))
    return Q / -(pi * np.diag(Q)).sum(), pi


def eig(ex, pi):
    Q, pi = build_q(ex, pi)
    sp = np.sqrt(pi)
    B = sp[:, None] * Q / sp[None, :]
    lam, V = np.linalg.eigh(0.5 * (B + B.T))
    lam, V = lam[::-1], V[:, ::-1]
    return Q, pi, lam, V / sp[:, None], V.T * sp[None, :]


def oracle_model(po, ex, pi):
    Q, pi, lam, U, Uinv = eig(ex, pi)
    m = po.Model.__new__(po.Model)
    m.s = po._ModelStruct()
    for name, arr in (("pi", pi), ("Q", Q), ("eval", lam), ("U", U), ("Uinv", Uinv)):
        flat = np.ascontiguousarray(arr, dtype=np.float64).ravel()
        setattr(m.s, name, (C.c_double * flat.size)(*flat))
    m.ptr = C.cast(C.byref(m.s), C.c_void_p)
    m.pi, m.Q, m.eval, m.U, m.Uinv = pi, Q, lam, U, Uinv
    return m


def simulate(ex, pi, ntax, nsites, seed, alpha=0.8, missing_frac=0.0):
    """synth.simulate_alignment's scheme under an arbitrary reversible matrix (4 rate categories)"""
    rng = np.random.default_rng(seed)
    names = ["t%d" % i for i in range(ntax)]
    newick, kids, blen, root = synth.random_tree(ntax, rng, names)
    _, pi, lam, U, Uinv = eig(ex, pi)
    rates = synth.gamma_mean_rates(alpha, 4)
    cat = rng.integers(0, 4, nsites)
    states = {root: rng.choice(20, size=nsites, p=pi)}
    stack = [root]
    while stack:
        v = stack.pop()
        if v < ntax:
            continue
        for c in kids[v]:
            out = np.empty(nsites, dtype=np.int64)
            u = rng.random(nsites)
            for k in range(4):
                idx = np.nonzero(cat == k)[0]
                P = np.clip((U * np.exp(lam * rates[k] * blen[c])[None, :]) @ Uinv, 0, None)
                cum = np.cumsum(P, axis=1)
                cum /= cum[:, -1:]
                out[idx] = (u[idx, None] > cum[states[v][idx]]).sum(1)
            states[c] = np.minimum(out, 19)
            stack.append(c)
    aa = np.frombuffer(synth.AA.encode(), dtype=np.uint8)
    rows = []
    for i in range(ntax):
        r = aa[states[i]].copy()
        if missing_frac > 0:
            for b in range(max(1, nsites // 50)):
                if rng.random() < missing_frac:
                    r[b * 50:(b + 1) * 50] = ord("?")
            r[rng.random(nsites) < missing_frac * 0.1] = ord("-")
        rows.append(r.tobytes().decode())
    return names, rows, newick


def _wag():
    d = json.load(open(os.path.join(ROOT, "tests", "golden", "wag_constants.json")))
    return np.array(d["S_lower"]), np.array(d["pi_raxml_3dp"])


def test_registered_wag_equals_builtin(gpu_ctx):
    ex, pi = _wag()
    code = gpu_ctx.register_matrix("wag", ex, pi)
    assert code >= 16 and code % 2 == 0
    assert gpu_ctx.register_matrix("wag", ex, pi) == code + 2          # a new code, nothing replaced
    names, rows, nw = synth.simulate_alignment(12, 500, 4100, missing_frac=0.1)
    a = gpu_ctx.score([(names, rows)], [nw], alpha=0.7, site_lnl=True)[0]
    b = gpu_ctx.score([(names, rows)], [nw], alpha=0.7, pi_mode=code, site_lnl=True)[0]
    assert abs(a["lnl"] - b["lnl"]) < 1e-12 * abs(a["lnl"])
    assert np.abs(a["site_lnl"] - b["site_lnl"]).max() < 1e-12 * np.abs(a["site_lnl"]).max()
    # the F variant of the registered matrix is PROTGAMMAWAGF
    f = gpu_ctx.score([(names, rows)], [nw], alpha=0.7, pi_mode=code + 1)[0]
    g = gpu_ctx.score([(names, rows)], [nw], alpha=0.7, pi_mode=engine.PI_EMPIRICAL)[0]
    assert abs(f["lnl"] - g["lnl"]) < 1e-11 * abs(g["lnl"]) and abs(f["lnl"] - a["lnl"]) > 1e-3


def test_random_matrix_vs_oracle(gpu_ctx, oracle_lib):
    po = oracle_lib
    ex, pi = random_matrix(11)
    code = gpu_ctx.register_matrix("rnd", ex, pi)
    names, rows, nw = simulate(ex, pi, 12, 600, 4200, missing_frac=0.2)
    gene = (names, rows)
    a = po.Alignment(names, rows)
    e = po.Engine(a, oracle_model(po, ex, pi), 4, 0.7)
    ref, refs = e.site_lnl(po.Tree(nw, a))
    r = gpu_ctx.score([gene], [nw], alpha=0.7, pi_mode=code, site_lnl=True)[0]
    assert abs(r["lnl"] - ref) < 1e-9 * abs(ref) and np.abs(r["site_lnl"] - refs).max() < 1e-9
    w = gpu_ctx.score([gene], [nw], alpha=0.7)[0]
    assert abs(w["lnl"] - ref) > 1.0                                     # not WAG under another name
    # optimise
    e = po.Engine(a, oracle_model(po, ex, pi), 4, 1.0)
    t = po.Tree(nw, a)
    oref = e.optimize(t, True, 1e-4)
    o = gpu_ctx.optimize([gene], [nw], pi_mode=code)[0]
    assert abs(o["lnl"] - oref) < 1e-3 and abs(o["alpha"] - e.alpha) < 1e-4 * max(1.0, e.alpha)
    # NNI search from the NJ tree
    e = po.Engine(a, oracle_model(po, ex, pi), 4, 1.0)
    sref, tref = e.search(None, 0, 1e-3)
    s = gpu_ctx.search([gene], None, pi_mode=code, spr_radius=0, epsilon=1e-3)[0]
    assert rf_collapsed(s["newick"], tref.newick()) == 0 and abs(s["lnl"] - sref) < 1e-3
    # F variant: the same exchangeabilities, frequencies counted from the alignment
    fm = oracle_model(po, ex, po.empirical_freqs(a))
    fref = po.Engine(a, fm, 4, 0.7).lnl(po.Tree(nw, a))
    f = gpu_ctx.score([gene], [nw], alpha=0.7, pi_mode=code + 1)[0]
    assert abs(f["lnl"] - fref) < 1e-9 * abs(fref) and abs(fref - ref) > 1e-3


def test_three_matrices_in_one_batch(gpu_ctx):
    mats = [random_matrix(21 + i) for i in range(3)]
    genes = [simulate(mats[i][0], mats[i][1], 7 + 2 * i, 300 + 100 * i, 4300 + i) for i in range(3)]
    G = [(g[0], g[1]) for g in genes]
    NW = [g[2] for g in genes]
    b = engine.Batch(gpu_ctx, G, NW, alpha=0.9)
    for i in range(3):
        b.set_matrix(mats[i][0], mats[i][1], g=i)
    together = b.score()
    tex = [b.get_matrix(i) for i in range(3)]
    b.close()
    for i in range(3):
        assert np.array_equal(tex[i][0], mats[i][0]) and np.allclose(tex[i][1], mats[i][1], rtol=1e-15, atol=0)
        s = engine.Batch(gpu_ctx, [G[i]], [NW[i]], alpha=0.9)
        s.set_matrix(mats[i][0], mats[i][1])
        assert s.score()[0] == together[i]
        s.close()


def _degenerate_inputs():
    rng = np.random.default_rng(5)
    pi_floor = np.full(20, 1.0)
    pi_floor[7] = 0.001 * 19 / 0.999
    return [(np.ones(190), np.full(20, 0.05)),                          # a 19-fold eigenvalue
            (np.exp(rng.normal(0, 1, 190)), pi_floor / pi_floor.sum()),  # one frequency at the 0.001 floor
            (10.0 ** rng.uniform(-4, 4, 190), random_matrix(6)[1])]      # exchangeabilities over eight decades


def test_model_build_kernel_accuracy_and_determinism(gpu_ctx):
    mats = [random_matrix(100 + i) for i in range(64)] + _degenerate_inputs()
    EX, PI = np.array([m[0] for m in mats]), np.array([m[1] for m in mats])
    out, raw = gpu_ctx.debug_model_build(EX, PI)
    ld = np.longdouble
    for (ex, pi), m in zip(mats, out):
        Q, pn = build_q(ex.astype(ld), pi.astype(ld), ld)
        U, Ui, lam = m["U"].astype(ld), m["Uinv"].astype(ld), m["eval"].astype(ld)
        assert np.abs((U * lam[None, :]) @ Ui - Q).max() <= 1e-13 * np.abs(Q).max()
        assert np.abs(Ui @ U - np.eye(20)).max() <= 1e-13
        assert abs(lam[0]) <= 1e-13 * np.abs(lam).max() and np.all(np.diff(m["eval"]) <= 0)
        assert np.array_equal(m["UinvT"], m["Uinv"].T) and np.abs(m["pi"] - pn.astype(np.float64)).max() < 1e-16
        for t in (1e-6, 0.1, 10.0):
            P = (U * np.exp(lam * t)[None, :]) @ Ui
            assert np.abs(P.sum(1) - 1).max() <= 1e-13
    perm = np.random.default_rng(9).permutation(len(mats))
    _, raw2 = gpu_ctx.debug_model_build(EX[perm], PI[perm])
    assert np.array_equal(raw2, raw[perm])
    _, raw3 = gpu_ctx.debug_model_build(EX[:1], PI[:1])
    assert np.array_equal(raw3[0], raw[0])
    assert gpu_ctx.kernel_stats()["model"]["launches"] >= 3


def test_replayed_plan_sees_a_model_change(gpu_ctx):
    genes = [synth.simulate_alignment(9, 400, 4400 + i) for i in range(3)]
    G = [(g[0], g[1]) for g in genes]
    NW = [g[2] for g in genes]
    ex, pi = random_matrix(31)
    for pm in (engine.PI_RAXML_3DP, engine.PI_EMPIRICAL):               # a shared-model batch and a per-gene one
        b = engine.Batch(gpu_ctx, G, NW, alpha=0.8, pi_mode=pm)
        first = b.score()
        assert np.array_equal(b.score(), first)                          # the second call replays the recorded plan
        b.set_matrix(ex, pi, g=1)
        after = b.score()
        again = b.score()
        site = b.site_lnl(1, len(G[1][1][0]))
        b.close()
        f = engine.Batch(gpu_ctx, [G[1]], [NW[1]], alpha=0.8, pi_mode=pm)
        f.set_matrix(ex, pi)
        fresh = f.score()[0]
        f.close()
        assert after[1] == fresh and abs(after[1] - first[1]) > 1e-3 and abs(site.sum() - fresh) < 1e-9 * abs(fresh)
        assert after[0] == first[0] and after[2] == first[2] and np.array_equal(again, after)


@pytest.fixture(scope="module")
def gtr_case(gpu_ctx):
    ex, pi = random_matrix(41)
    names, rows, nw = simulate(ex, pi, 8, 20000, 4500)
    code = gpu_ctx.register_matrix("truth", ex, pi)
    gene = (names, rows)
    import time
    t0 = time.time()
    alone = gpu_ctx.optimize([gene], [nw], pi_mode=engine.PI_GTR, epsilon=EPS_GTR)[0]
    print("GTR optimise, 8 taxa x 20000 sites: %.2f s" % (time.time() - t0))
    return {"ex": ex, "pi": pi, "gene": gene, "nw": nw, "code": code, "alone": alone}


def test_gtr_estimates_rates(gpu_ctx, oracle_lib, gtr_case):
    po, c = oracle_lib, gtr_case
    gene, nw = c["gene"], c["nw"]
    truth = gpu_ctx.optimize([gene], [nw], pi_mode=c["code"], epsilon=EPS_GTR)[0]
    wag = gpu_ctx.optimize([gene], [nw], epsilon=EPS_GTR)[0]
    assert c["alone"]["lnl"] >= truth["lnl"] - 0.5 and c["alone"]["lnl"] > wag["lnl"] + 10
    # the returned matrix, tree and alpha reproduce the reported likelihood in the oracle
    b = engine.Batch(gpu_ctx, [gene], [nw], pi_mode=engine.PI_GTR)
    wag_start = b.score()[0]
    lnl, al = b.optimize(epsilon=EPS_GTR)
    ex, pi = b.get_matrix(0)
    tree = b.newick(0, 17)
    b.close()
    assert lnl[0] == c["alone"]["lnl"] and al[0] == c["alone"]["alpha"]      # a second run returns the same bits
    assert ex[189] == 1.0 and np.all(ex >= 1e-7) and np.all(ex <= 1e6) and abs(pi.sum() - 1) < 1e-14
    a = po.Alignment(*gene)
    assert np.allclose(pi, po.empirical_freqs(a) / po.empirical_freqs(a).sum(), rtol=1e-12, atol=0)
    ref = po.Engine(a, oracle_model(po, ex, pi), 4, al[0]).lnl(po.Tree(tree, a))
    assert abs(ref - lnl[0]) < 1e-6 * abs(ref)
    # a non-optimising call scores under the start matrix: WAG exchangeabilities, empirical frequencies
    wf = gpu_ctx.score([gene], [nw], pi_mode=engine.PI_EMPIRICAL)[0]
    assert abs(wag_start - wf["lnl"]) < 1e-9 * abs(wf["lnl"])
    # composition independence: inside a batch of three
    others = [simulate(*random_matrix(42 + i), 6 + i, 700, 4510 + i) for i in range(2)]
    three = gpu_ctx.optimize([(others[0][0], others[0][1]), gene, (others[1][0], others[1][1])], [others[0][2], nw, others[1][2]],
                             pi_mode=engine.PI_GTR, epsilon=EPS_GTR)
    assert three[1]["lnl"] == c["alone"]["lnl"] and three[1]["newick"] == c["alone"]["newick"]


def test_model_eval_is_one_batch_of_optimize_calls(gpu_ctx, gtr_case):
    c = gtr_case
    gene, nw = c["gene"], c["nw"]
    codes = [engine.PI_RAXML_3DP, engine.PI_EMPIRICAL, c["code"], engine.PI_GTR]
    import time
    t0 = time.time()
    res, best = gpu_ctx.model_eval(gene, nw, codes, epsilon=EPS_GTR)
    print("model_eval over 4 codes, 8 taxa x 20000 sites: %.2f s" % (time.time() - t0))
    assert best in (2, 3) and best == int(np.argmax([r["lnl"] for r in res]))
    for code, r in zip(codes, res):
        one = c["alone"] if code == engine.PI_GTR else gpu_ctx.optimize([gene], [nw], pi_mode=code, epsilon=EPS_GTR)[0]
        assert r["lnl"] == one["lnl"] and r["alpha"] == one["alpha"] and r["newick"] == one["newick"], code


def test_shim_models_and_jackknife_entry_check(gpu_ctx, tmp_path):
    ex, pi = random_matrix(51)
    names, rows, nw = simulate(ex, pi, 8, 400, 4600)
    (tmp_path / "g.phy").write_text("%d %d\n" % (len(names), len(rows[0])) + "".join("%s %s\n" % (n, r) for n, r in zip(names, rows)))
    (tmp_path / "in.nwk").write_text(nw + "\n")
    mdir = tmp_path / "models"
    mdir.mkdir()
    (mdir / "lg.dat").write_text(paml_text(ex, pi, "\nnot LG: a random test matrix\n"))
    env = {k: v for k, v in os.environ.items() if k != "PEPRML_MODEL_DIR"}

    def run(m, e):
        return subprocess.run([RX, "-f", "e", "-m", m, "-s", "g.phy", "-n", m + str(len(e)), "-t", "in.nwk"], cwd=tmp_path, env=e,
                              capture_output=True, text=True, timeout=600)

    def lnl(m, e):
        info = (tmp_path / ("RAxML_info." + m + str(len(e)))).read_text()
        return float([l for l in info.splitlines() if "Final GAMMA" in l][0].split()[-1]), info
    p = run("PROTGAMMAGTR", env)
    assert p.returncode == 0, p.stderr
    assert "parity unpinned" in lnl("PROTGAMMAGTR", env)[1]
    for m in ("PROTGAMMALG", "PROTGAMMALGF"):
        p = run(m, env)
        assert p.returncode != 0 and "PROTGAMMAWAG" in p.stderr
    env2 = dict(env, PEPRML_MODEL_DIR=str(mdir))
    got = {}
    for m in ("PROTGAMMALG", "PROTGAMMALGF"):
        p = run(m, env2)
        assert p.returncode == 0, p.stderr
        got[m], info = lnl(m, env2)
        assert "lg.dat" in info and "parity unpinned" in info
    assert abs(got["PROTGAMMALG"] - got["PROTGAMMALGF"]) > 1e-3
    code = gpu_ctx.register_matrix("lg", ex, pi)
    assert abs(gpu_ctx.optimize([(names, rows)], [nw], pi_mode=code)[0]["lnl"] - got["PROTGAMMALG"]) < 1e-5
    for m in ("PROTGAMMAILG", "PROTCATLG", "PROTGAMMAJTT", "GTRGAMMA"):
        p = run(m, env2)
        assert p.returncode != 0 and "PROTGAMMAWAG" in p.stderr
    # gene-wise jackknife: one shared model per replicate
    genes = [synth.simulate_alignment(6, 120, 4700 + i)[:2] for i in range(4)]
    for pm, name in ((code + 1, "PROTGAMMALGF"), (engine.PI_GTR, "PROTGAMMAGTR"), (engine.PI_EMPIRICAL, "PROTGAMMAWAGF")):
        with pytest.raises(engine.PmlError) as e:
            gpu_ctx.jackknife(genes, reps=2, pi_mode=pm)
        assert e.value.code == -1 and name in str(e.value)
    r = gpu_ctx.jackknife(genes, reps=2, pi_mode=code)
    assert r["newick"] if isinstance(r, dict) else r
