"""pml_search2 on the device: RAxML's schedule (radius honoured up to 25 or determined on the start tree), the lazy SPR
score at depth through the door pml_debug_spr_scores, and the trace of accepted steps.

References: the CPU oracle's likelihood of trees the test builds itself (tests/spr_ref.py: SPR from the definition), and
pml_search_batch for the degenerate options.  Likelihood tolerances are the per-site tolerance of
test_gpu_parity.test_score_vs_oracle (1e-9 relative to the largest per-site |lnL|) times the number of sites."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import spr_ref
import util
from pepr_amd import _lib, engine, synth, tree_builder

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPR_MIN_GAIN = 0.01


def _tol(site_lnl):
    return 1e-9 * max(1.0, float(np.abs(site_lnl).max())) * len(site_lnl)


def _oracle_lnl(po, names, rows, nw, alpha=1.0, ncat=4):
    a = po.Alignment(names, rows)
    e = po.Engine(a, po.Model(0), ncat, alpha)
    tot, sites = e.site_lnl(po.Tree(nw, a))
    return tot, _tol(sites)


def _caterpillar(names, rng):
    """a caterpillar over the names in random order with random lengths: paths of every depth up to ntax - 3"""
    order = [names[i] for i in rng.permutation(len(names))]
    ln = lambda: "%.6f" % rng.uniform(0.02, 0.3)
    nw = "(%s:%s,%s:%s)" % (order[0], ln(), order[1], ln())
    for x in order[2:-1]:
        nw = "(%s:%s,%s:%s)" % (nw, ln(), x, ln())
    return "(%s,%s:%s);" % (nw[1:-1], order[-1], ln()), order


# ---- 1. old bits ---------------------------------------------------------------------------------
def _same(a, b):
    return a["lnl"] == b["lnl"] and a["alpha"] == b["alpha"] and a["newick"] == b["newick"]


def test_degenerate_options_give_pml_search_bits(gpu_ctx):
    genes = [synth.simulate_alignment(nt, ns, 800 + i)[:2] for i, (nt, ns) in enumerate([(12, 150), (17, 90), (9, 260)])]
    cons = engine.constraints_from_tree(synth.simulate_alignment(12, 150, 800)[2])
    cases = [dict(nni=True, spr_radius=0), dict(nni=True, spr_radius=5), dict(nni=True, spr_radius=5, seed=7),
             dict(nni=True, spr_radius=5, constraints=cons)]
    for kw in cases:
        gs = genes[:1] if "constraints" in kw else genes
        old = gpu_ctx.search(gs, None, **kw)
        kw2 = dict(kw)
        radius = kw2.pop("spr_radius")
        new, tr = gpu_ctx.search2(gs, None, radius=radius, trace=True, **kw2)
        for o, n in zip(old, new):
            assert _same(o, n), kw
        for i, g in enumerate(gs):                    # alone = in the batch
            alone = gpu_ctx.search2([g], None, radius=radius, **kw2)[0]
            assert _same(alone, new[i]), (kw, i)
        assert all(t["radius_chosen"] == radius and t["trial_radius"] == [] for t in tr)


def test_argument_checks(gpu_ctx):
    L = _lib.load()
    keep = []
    names, rows, _ = synth.simulate_alignment(6, 20, 1)
    aln = engine._aln_struct(names, rows, keep)
    m = engine._model()

    def rc(opts):
        res = _lib.Result()
        r = L.pml_search2_batch(gpu_ctx.ptr, 1, C.byref(aln), None, C.byref(m), opts, C.byref(res), None)
        L.pml_result_free(C.byref(res))
        return r

    def o2(radius=5, mode=0, step=0, rmax=0, thorough=0):
        o = _lib.SearchOpts2()
        o.base = engine._opts(True, True, radius, 1e-3)
        o.radius_mode, o.radius_step, o.radius_max, o.thorough = mode, step, rmax, thorough
        return C.byref(o)
    assert rc(o2()) == 0 and rc(o2(radius=25)) == 0 and rc(o2(mode=1, step=5, rmax=25)) == 0
    assert rc(o2(radius=26)) == -1 and b"clamp" in L.pml_last_error(gpu_ctx.ptr)
    assert rc(o2(mode=1, rmax=30)) == -1
    assert rc(o2(mode=1, step=-1)) == -1
    assert rc(o2(mode=2)) == -1
    assert rc(None) == -1


# ---- 2. lazy scores at depth ---------------------------------------------------------------------
def _check_lazy(gpu_ctx, po, names, rows, nw, pruned, rmin, rmax, alpha, ncat, want_depth):
    t = spr_ref.UTree(nw)
    p, s = t.node_behind(pruned)
    got = gpu_ctx.debug_spr_scores((names, rows), nw, sorted(pruned), rmin, rmax, alpha=alpha, ncat=ncat)
    ref = spr_ref.candidates(t, p, s, rmin, rmax)
    assert {(far, d) for far, d, _, _ in got} == set(ref) and len(got) == len(ref)
    assert max(d for _, d, _, _ in got) >= want_depth
    assert any(len(far) == 1 for far, _, _, _ in got), "no tip edge among the candidates"
    worst = 0.0
    for far, d, lazy, _ in got:
        g, h = ref[(far, d)]
        want, tol = _oracle_lnl(po, names, rows, spr_ref.regraft_lazy(t, p, s, g, h).newick("%.17g"), alpha, ncat)
        worst = max(worst, abs(lazy - want) / tol)
        assert abs(lazy - want) < tol, (sorted(far), d, lazy, want, tol)
    return worst


@pytest.mark.parametrize("ncat", [4, 1])
def test_lazy_scores_at_depth(gpu_ctx, oracle_lib, ncat):
    names, rows, _ = synth.simulate_alignment(30, 96, 811)
    nw, order = _caterpillar(names, np.random.default_rng(5))
    # one end of the longest path: the first leaf of the caterpillar (a pruned tip), and the cherry-plus-one clade at that end
    _check_lazy(gpu_ctx, oracle_lib, names, rows, nw, [order[0]], 1, 25, 0.7, ncat, 25)
    _check_lazy(gpu_ctx, oracle_lib, names, rows, nw, order[:3], 1, 25, 0.7, ncat, 24)
    _check_lazy(gpu_ctx, oracle_lib, names, rows, nw, [order[0]], 21, 25, 0.7, ncat, 25)
    _check_lazy(gpu_ctx, oracle_lib, names, rows, nw, order[-4:], 6, 10, 0.7, ncat, 10)


def test_lazy_scores_with_scaled_clvs(gpu_ctx, oracle_lib):
    names, rows, _ = synth.simulate_alignment(120, 32, 812)
    nw, order = _caterpillar(names, np.random.default_rng(6))
    _check_lazy(gpu_ctx, oracle_lib, names, rows, nw, order[:2], 1, 25, 0.9, 4, 25)
    _check_lazy(gpu_ctx, oracle_lib, names, rows, nw, [order[60]], 1, 25, 0.9, 4, 25)


def test_score_door_argument_checks(gpu_ctx):
    names, rows, nw = synth.simulate_alignment(8, 40, 3)
    with pytest.raises(engine.PmlError):
        gpu_ctx.debug_spr_scores((names, rows), nw, ["t0"], 1, 26)
    with pytest.raises(engine.PmlError):
        gpu_ctx.debug_spr_scores((names, rows), nw, ["t0", "nope"], 1, 5)


# ---- 3. thorough insertion -----------------------------------------------------------------------
class _TS(C.Structure):
    _fields_ = [("ntax", C.c_int), ("nnodes", C.c_int), ("nbr", C.POINTER(C.c_int * 3)), ("len", C.POINTER(C.c_double * 3))]


def _oracle_node_behind(t, names, pruned):
    """(p, [its three neighbours]) in the oracle's numbering (tip i = names[i]): p's neighbour s has exactly `pruned` behind it"""
    ts = C.cast(t.ptr, C.POINTER(_TS)).contents

    def behind(v, frm):
        if v < ts.ntax:
            return {names[v]}
        return set().union(*[behind(ts.nbr[v][q], v) for q in range(3) if ts.nbr[v][q] != frm])
    for p in range(ts.ntax, ts.nnodes):
        for q in range(3):
            if behind(ts.nbr[p][q], p) == set(pruned):
                return p, [ts.nbr[p][k] for k in range(3)], [ts.len[p][k] for k in range(3)]
    raise KeyError(pruned)


def _check_thorough(gpu_ctx, po, names, rows, nw, pruned, alpha, ncat):
    """thorough score = the oracle's lnL of the tree with the three returned lengths; never below the lazy score; and on each
    of the three branches the oracle's derivatives leave a Newton step less than 1e-3 lnL to gain (d1^2 / 2|d2|), a tenth
    of SPR_MIN_GAIN.  A branch that sits on the lower length bound 1e-6 with the likelihood still rising towards zero has
    nowhere to go: its derivative is not a remaining gain."""
    t = spr_ref.UTree(nw)
    p, s = t.node_behind(pruned)
    got = gpu_ctx.debug_spr_scores((names, rows), nw, sorted(pruned), 1, 25, alpha=alpha, ncat=ncat, thorough_top=4)
    ref = spr_ref.candidates(t, p, s, 1, 25)
    done = [c for c in got if c[3] is not None]
    best4 = sorted(got, key=lambda c: -c[2])[:4]
    assert len(done) == 4 and {c[0] for c in done} == {c[0] for c in best4}
    a = po.Alignment(names, rows)
    e = po.Engine(a, po.Model(0), ncat, alpha)
    for far, d, lazy, (score, ts_, tg, th) in done:
        g, h = ref[(far, d)]
        n = spr_ref.regraft_lazy(t, p, s, g, h)
        for w, l in ((s, ts_), (g, tg), (h, th)):
            n.adj[p][w] = n.adj[w][p] = l
        ot = po.Tree(n.newick("%.17g"), a)
        want, sites = e.site_lnl(ot)
        tol = _tol(sites)
        print("thorough", sorted(pruned)[:2], d, "lazy", lazy, "thorough", score, "oracle", want, "lengths", ts_, tg, th)
        assert abs(score - want) < tol, (score, want, tol)
        assert score >= lazy - tol
        op, nbrs, lens = _oracle_node_behind(ot, names, pruned)
        for w, l in zip(nbrs, lens):
            _, d1, d2 = e.branch_derivs(ot, op, w)
            gain = d1 * d1 / (2 * abs(d2)) if d2 != 0 else float("inf")
            print("   branch", l, "d1", d1, "d2", d2, "gain", gain)
            assert gain < 1e-3 or (l <= 1.0001e-6 and d1 < 0), (l, d1, d2, gain)


@pytest.mark.parametrize("ncat", [4, 1])
def test_thorough_insertion(gpu_ctx, oracle_lib, ncat):
    names, rows, _ = synth.simulate_alignment(30, 96, 811)
    nw, order = _caterpillar(names, np.random.default_rng(5))
    _check_thorough(gpu_ctx, oracle_lib, names, rows, nw, [order[0]], 0.7, ncat)
    _check_thorough(gpu_ctx, oracle_lib, names, rows, nw, order[:3], 0.7, ncat)


def test_thorough_insertion_scaled_clvs(gpu_ctx, oracle_lib):
    names, rows, _ = synth.simulate_alignment(120, 32, 812)
    nw, order = _caterpillar(names, np.random.default_rng(6))
    _check_thorough(gpu_ctx, oracle_lib, names, rows, nw, [order[60]], 0.9, 4)


# ---- 4. the trace --------------------------------------------------------------------------------
def _perturbed(nw, seed, nmoves=3, mind=9):
    """the tree with nmoves leaves regrafted at least mind edges away"""
    rng = np.random.default_rng(seed)
    t = spr_ref.UTree(nw)
    moved = 0
    for leaf in rng.permutation(sorted(t.name.values())):
        p, s = t.node_behind([leaf])
        far = sorted(spr_ref.candidates(t, p, s, mind, 99).items(), key=lambda kv: (kv[0][1], sorted(kv[0][0])))
        if not far:
            continue
        (_, d), (g, h) = far[int(rng.integers(len(far)))]
        t = spr_ref.regraft_lazy(t, p, s, g, h)
        moved += 1
        if moved == nmoves:
            return t.newick()
    raise AssertionError("the tree has no path of %d edges" % mind)


@pytest.fixture(scope="module")
def traced(gpu_ctx):
    """24 taxa x 200 sites, seed 700: the oracle puts the optimised start tree 695 lnL below the optimised generating tree
    (-4912.61 against -4217.91, checked on the CPU before the seed was committed), far more than SPR_MIN_GAIN"""
    names, rows, nw = synth.simulate_alignment(24, 200, 700)
    start = _perturbed(nw, 700)
    # alpha stays at 1 so that every step's lnL can be recomputed from its tree alone
    res, tr = gpu_ctx.search2([(names, rows)], [start], radius=12, nni=False, optimize_alpha=False, trace=True)
    return names, rows, nw, start, res[0], tr[0]


def test_trace_is_true(gpu_ctx, oracle_lib, traced):
    names, rows, nw, start, res, tr = traced
    steps = tr["steps"]
    assert tr["radius_chosen"] == 12 and tr["trial_radius"] == []
    assert len(steps) >= 1 and any(s["phase"] == 1 for s in steps)
    prev_lnl, prev_tree = tr["lnl_start"], spr_ref.UTree(start)
    for s in steps:
        want, tol = _oracle_lnl(oracle_lib, names, rows, s["newick_after"], 1.0, 4)
        # newick_after carries 12 significant digits per length: 46 branches, |dlnL/dt| of a few hundred at most
        assert abs(s["lnl_after"] - want) < tol + 1e-7, (s["phase"], s["lnl_after"], want)
        assert s["lnl_after"] > s["lnl_before"] and s["lnl_before"] >= prev_lnl - 1e-9 and s["lnl_after"] > prev_lnl
        after = spr_ref.UTree(s["newick_after"])
        if s["phase"] == 1:
            assert (s["rmin"], s["rmax"]) == (1, 12) and 1 <= s["distance"] <= 12
            assert s["distance"] in spr_ref.spr_distance(prev_tree, after, s["distance"], s["distance"]), s
        else:
            assert (s["rmin"], s["rmax"], s["distance"]) == (0, 0, 0)
        prev_lnl, prev_tree = s["lnl_after"], after
    assert steps[-1]["lnl_after"] >= tr["lnl_start"] and res["lnl"] >= steps[-1]["lnl_after"] - 1e-6
    sc = gpu_ctx.score([(names, rows)], [res["newick"]], alpha=res["alpha"])[0]
    assert abs(sc["lnl"] - res["lnl"]) < 1e-9 * abs(res["lnl"])
    assert spr_ref.split_set(spr_ref.UTree(res["newick"])) == spr_ref.split_set(prev_tree)


# ---- 5. AUTO -------------------------------------------------------------------------------------
def _auto_rule(lnl_start, radii, lnls, step, rmax):
    """-> (chosen radius, number of trials) the rule of peprml.h gives for the recorded trial likelihoods"""
    best, chosen = lnl_start, step
    for i, (r, l) in enumerate(zip(radii, lnls)):
        if l > best:
            best, chosen = l, r
        else:
            return chosen, i + 1
    return chosen, len(radii)


def test_auto_radius(gpu_ctx):
    genes, starts = [], []
    for i, (nt, ns) in enumerate([(24, 200), (14, 120), (30, 96)]):
        names, rows, nw = synth.simulate_alignment(nt, ns, 700 + i)
        genes.append((names, rows))
        starts.append(_perturbed(nw, 700 + i, mind=9 if nt >= 24 else 5))
    res, trs = gpu_ctx.search2(genes, starts, radius="auto", optimize_alpha=False, trace=True)
    for tr in trs:
        n = len(tr["trial_radius"])
        assert n >= 1 and tr["trial_radius"] == [5 * (k + 1) for k in range(n)] and n <= 5
        chosen, ntr = _auto_rule(tr["lnl_start"], tr["trial_radius"], tr["trial_lnl"], 5, 25)
        assert (tr["radius_chosen"], n) == (chosen, ntr), tr
        assert all(s["rmax"] == tr["radius_chosen"] and s["rmin"] == 1 for s in tr["steps"] if s["phase"] == 1)
    # a gene alone takes the same decisions and ends with the same bits, trace included
    r1, t1 = gpu_ctx.search2(genes[:1], starts[:1], radius="auto", optimize_alpha=False, trace=True)
    assert _same(r1[0], res[0]) and t1[0] == trs[0]
    # other step / maximum
    r2, t2 = gpu_ctx.search2(genes[:1], starts[:1], radius="auto", radius_step=4, radius_max=9, optimize_alpha=False, trace=True)
    assert t2[0]["trial_radius"] in ([4], [4, 8]) and t2[0]["radius_chosen"] in (4, 8)


# ---- 6. thorough windows -------------------------------------------------------------------------
def test_thorough_windows(gpu_ctx, oracle_lib):
    names, rows, nw = synth.simulate_alignment(24, 200, 700)
    start = _perturbed(nw, 700)
    kw = dict(radius=5, nni=False, optimize_alpha=False, thorough=True, thorough_top=3, radius_step=4, thorough_radius_max=12, trace=True)
    res, tr = gpu_ctx.search2([(names, rows)], [start], **kw)
    fast, _ = gpu_ctx.search2([(names, rows)], [start], radius=5, nni=False, optimize_alpha=False, trace=True)
    steps = [s for s in tr[0]["steps"] if s["phase"] == 2]
    print("thorough steps", [(s["rmin"], s["rmax"], s["distance"], s["lnl_after"]) for s in steps], "fast only", fast[0]["lnl"], "with thorough", res[0]["lnl"])
    assert all(s["phase"] in (0, 1, 2) for s in tr[0]["steps"])
    seen2 = False
    prev = None
    for s in tr[0]["steps"]:
        if s["phase"] == 2:
            seen2 = True
            assert s["rmin"] <= s["distance"] <= s["rmax"] <= 12
            assert (s["rmin"] - 1) % 4 == 0 and s["rmax"] == s["rmin"] + 3
            assert prev is None or (s["rmin"], s["rmax"]) in (prev, (1, 4)), (prev, s["rmin"], s["rmax"])      # same cycle, or reset
            prev = (s["rmin"], s["rmax"])
            want, tol = _oracle_lnl(oracle_lib, names, rows, s["newick_after"], 1.0, 4)
            assert abs(s["lnl_after"] - want) < tol + 1e-7 and s["lnl_after"] > s["lnl_before"]
        else:
            assert not seen2, "a fast-phase step after the thorough phase began"
    assert res[0]["lnl"] >= fast[0]["lnl"] - 1e-3        # both end with an optimisation to epsilon 1e-3
    again, tr2 = gpu_ctx.search2([(names, rows)], [start], **kw)
    assert _same(again[0], res[0]) and tr2 == tr
    others = [synth.simulate_alignment(nt, ns, 840 + nt)[:2] for nt, ns in [(11, 150), (27, 70)]]
    mixed, tr3 = gpu_ctx.search2([others[0], (names, rows), others[1]], [None, start, None], **kw)
    assert _same(mixed[1], res[0]) and tr3[1] == tr[0]


# ---- 7. determinism ------------------------------------------------------------------------------
def test_same_call_twice_and_batch_composition(gpu_ctx, traced):
    names, rows, nw, start, res, tr = traced
    others = [synth.simulate_alignment(nt, ns, 820 + nt)[:2] for nt, ns in [(9, 300), (31, 64)]]
    again, tr2 = gpu_ctx.search2([(names, rows)], [start], radius=12, nni=False, optimize_alpha=False, trace=True)
    assert _same(again[0], res) and tr2[0] == tr
    mixed, tr3 = gpu_ctx.search2([others[0], (names, rows), others[1]], [None, start, None], radius=12, nni=False, optimize_alpha=False, trace=True)
    assert _same(mixed[1], res) and tr3[1] == tr


# ---- 8. constraints at radius 25 -----------------------------------------------------------------
def test_constraints_at_radius_25(gpu_ctx):
    names, rows, nw = synth.simulate_alignment(30, 96, 811)
    sp = util.splits(nw)
    rng = np.random.default_rng(3)
    while True:                                     # a clade the generating tree does not have
        clade = frozenset(rng.choice(names, 5, replace=False))
        if clade not in sp and frozenset(names) - clade not in sp:
            break
    cons = (list(names), ["1" if t in clade else "0" for t in names])
    cat, _ = _caterpillar(names, np.random.default_rng(8))
    r = gpu_ctx.search2([(names, rows)], [cat], radius=25, constraints=cons)[0]
    got = util.splits(r["newick"])
    assert clade in got or frozenset(names) - clade in got
    free = gpu_ctx.search2([(names, rows)], [cat], radius=25)[0]
    assert free["lnl"] > r["lnl"]


# ---- 9. mirror and shim --------------------------------------------------------------------------
def test_mirror_schedule(gpu_ctx):
    names, rows, nw = synth.simulate_alignment(16, 150, 830)
    run = tree_builder.RAxMLRunner(ctx=gpu_ctx)
    run.setAlignment(tree_builder.SequenceAlignment(names, rows))
    run.setSearchSchedule("raxml")
    run.run()
    assert run.getBestTree() is not None and run.getRadiusChosen() in (5, 10, 15, 20, 25)
    # the start of the mirror's search: the parsimony tree of its seed.  If no move is accepted the two values are optima of
    # one topology found to epsilon 1e-3 and 1e-4: they differ by less than the sum
    start = gpu_ctx.optimize([(names, rows)], [gpu_ctx.parsimony([(names, rows)], seed=run.seed)[0]["newick"]])[0]
    assert run.lnl >= start["lnl"] - 1.1e-3


def test_shim_radius_option(tmp_path, gpu_ctx):
    names, rows, nw = synth.simulate_alignment(12, 120, 831)
    with open(tmp_path / "a.phy", "w") as f:
        f.write("%d %d\n" % (len(names), len(rows[0])))
        for n, r in zip(names, rows):
            f.write("%s %s\n" % (n, r))
    exe = os.path.join(ROOT, "bin", "raxmlHPC")
    r = subprocess.run([exe, "-f", "d", "-m", "PROTGAMMAWAG", "-s", "a.phy", "-n", "r10", "-p", "5", "-i", "10"], cwd=tmp_path,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    tree = open(tmp_path / "RAxML_bestTree.r10").read()
    assert sorted(spr_ref.UTree(tree).name.values()) == sorted(names)
    info = open(tmp_path / "RAxML_info.r10").read()
    assert "rearrangement radius: 10 (given with -i)" in info
    env = dict(os.environ, PEPRML_SEARCH_SCHEDULE="raxml")
    r = subprocess.run([exe, "-f", "d", "-m", "PROTGAMMAWAG", "-s", "a.phy", "-n", "auto", "-p", "5"], cwd=tmp_path,
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr
    assert "determined on the start tree" in open(tmp_path / "RAxML_info.auto").read()
