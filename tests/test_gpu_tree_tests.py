"""Tree selection tests on the device (k_rell, pml_rell_tests, pml_tree_tests, the runConsel mirror) against the numpy
restatement in tests/rell_ref.py.  Replicate sums are sequential double additions and the statistics are integer counts, so
everything the kernel produces is compared EXACTLY: np.array_equal on the sums, == on the counts."""
import re

import numpy as np
import pytest

import rell_ref
import util
from pepr_amd import engine, synth, tree_builder as tb

pytestmark = pytest.mark.gpu

LADDER = [0.5, 0.6, 0.7, 0.8, 0.9, 1.0, 1.1, 1.2, 1.3, 1.4]


def _ndraws(N, K, r):
    """K = 1: the scale r alone; K = 10: the ladder 0.5 ... 1.4 rotated to start at r (so k1 is not always index 5)"""
    sc = [r] if K == 1 else LADDER[LADDER.index(r):] + LADDER[:LADDER.index(r)]
    return rell_ref.default_ndraws(N, sc)


def _table(N, T, seed):
    rng = np.random.default_rng(seed)
    base = -rng.gamma(2.0, 1.5, size=N)
    X = base[None, :] + rng.normal(0.0, 0.15, size=(T, N)) - 0.002 * np.arange(T)[:, None]
    if T >= 4:
        X[3] = X[0]                       # a bit-identical duplicate: every argmax tie has to go to the lowest index
    return X


@pytest.mark.parametrize("N", [37, 400, 5000])
def test_kernel_bit_for_bit(gpu_ctx, N):
    """Y, bp, kh, sh of every shape N x T in {2, 5, 17, 64} x K in {1, 10} x B in {1, 257, 2000} x r in {0.5, 1.4}: tables on both
    sides of the LDS boundary, the path chosen by the library"""
    paths = {}
    for T in (2, 5, 17, 64):
        X = _table(N, T, 1000 * N + T)
        for K in (1, 10):
            for B in (1, 257, 2000):
                for r in (0.5, 1.4):
                    nd = _ndraws(N, K, r)
                    seed = N + 7 * T + 13 * K + B
                    got = gpu_ctx.debug_rell(X, nd, B, seed=seed)
                    Y = rell_ref.replicate_sums(X, nd, B, seed)
                    bp, kh, sh, k1 = rell_ref.counts(X, nd, B, seed, Y=Y)
                    tag = (N, T, K, B, r, got["path"])
                    assert np.array_equal(got["Y"], Y), tag
                    assert np.array_equal(got["bp"], bp) and np.array_equal(got["kh"], kh) and np.array_equal(got["sh"], sh), tag
                    assert np.all(got["bp"].sum(axis=1) == B), tag
                    paths[T] = got["path"]
    print("N = %d: path per T (1 = LDS, 2 = global): %s" % (N, paths))
    if N == 37:
        assert set(paths.values()) == {1}          # 37 rows fit whatever the width
    if N == 5000:
        assert paths[64] == 2 and paths[17] == 2   # 5000 x 33 and 5000 x 9 slots of 16 bytes are beyond any LDS


def test_both_paths_forced_same_bits(gpu_ctx):
    for N, T in ((400, 5), (37, 64), (400, 16)):
        X = _table(N, T, 99 + T)
        nd = _ndraws(N, 10, 0.5)
        ref = rell_ref.replicate_sums(X, nd, 300, 5)
        a = gpu_ctx.debug_rell(X, nd, 300, seed=5, path=1)
        b = gpu_ctx.debug_rell(X, nd, 300, seed=5, path=2)
        assert a["path"] == 1 and b["path"] == 2
        assert a["Y"].tobytes() == b["Y"].tobytes() == ref.tobytes()
        for f in ("bp", "kh", "sh"):
            assert np.array_equal(a[f], b[f])
    # a forced LDS path that does not fit is refused, not silently served from global memory
    with pytest.raises(engine.PmlError) as ei:
        gpu_ctx.debug_rell(_table(5000, 64, 1), [5000], 4, path=1)
    assert ei.value.code == -1


def test_rell_tests_counts_equal_reference(gpu_ctx):
    """pml_rell_tests: default ladder and n_k rule, counts equal as integers, p-values = counts / B, AU = the reference fit"""
    for N, T, B, seed in ((400, 5, 2000, 11), (37, 2, 257, 3), (5000, 17, 257, 4), (400, 64, 1, 9)):
        X = _table(N, T, 31 * N + T)
        got = gpu_ctx.rell_tests(X, reps=B, seed=seed)
        ref = rell_ref.tests(X, B, seed)
        assert np.array_equal(got["ndraws"], ref["ndraws"]) and got["k1"] == ref["k1"] == 5
        assert np.array_equal(got["bp_count"], ref["bp_count"])
        assert np.array_equal(got["kh_count"], ref["kh_count"]) and np.array_equal(got["sh_count"], ref["sh_count"])
        assert np.array_equal(got["lnl"], ref["lnl"])                               # column sums in site order, same bits
        assert np.array_equal(got["np"], ref["bp_count"][5] / B) and np.array_equal(got["bp"], got["np"])
        assert np.array_equal(got["kh"], ref["kh_count"] / B) and np.array_equal(got["sh"], ref["sh_count"] / B)
        assert np.abs(got["au"] - ref["au"]).max() <= 3e-13
        L = ref["lnl"]
        order = sorted(range(T), key=lambda t: (-L[t], t))
        assert [int(got["rank"][t]) for t in order] == list(range(1, T + 1))
        pp = np.exp(L - L.max()); pp /= pp.sum()
        assert np.allclose(got["pp"], pp, rtol=1e-12, atol=0)
        obs = np.array([np.max(np.delete(L, t)) - L[t] for t in range(T)])
        assert np.array_equal(got["obs"], obs)
    # scales given by the caller
    X = _table(400, 5, 77)
    got = gpu_ctx.rell_tests(X, scales=[1.3, 0.7, 1.0], reps=500, seed=2)
    ref = rell_ref.tests(X, 500, 2, scales=[1.3, 0.7, 1.0])
    assert got["k1"] == ref["k1"] == 2 and np.array_equal(got["bp_count"], ref["bp_count"])
    assert np.array_equal(got["kh_count"], ref["kh_count"]) and np.array_equal(got["sh_count"], ref["sh_count"])


def test_composition_and_determinism(gpu_ctx):
    X = _table(400, 5, 8)
    nd = _ndraws(400, 10, 0.5)
    a = gpu_ctx.debug_rell(X, nd, 2000, seed=21)
    b = gpu_ctx.debug_rell(X, nd, 2000, seed=21)
    assert a["Y"].tobytes() == b["Y"].tobytes()                                     # same seed -> same bytes
    for f in ("bp", "kh", "sh"):
        assert np.array_equal(a[f], b[f])
    c = gpu_ctx.debug_rell(X, nd, 257, seed=21)
    assert np.array_equal(c["Y"][0], a["Y"][0, :257])                               # replicates b < min(B) of scale 0 do not depend on B
    assert not np.array_equal(c["Y"][1], a["Y"][1, :257])                           # (the other scales are keyed by k B + b)
    d = gpu_ctx.debug_rell(X, nd, 2000, seed=22)
    assert not np.array_equal(d["Y"], a["Y"])
    # what else is in the launch does not matter: one scale alone = that scale among ten (scale 0: the same key)
    e = gpu_ctx.debug_rell(X, nd[:1], 2000, seed=21)
    assert np.array_equal(e["Y"][0], a["Y"][0])
    g = gpu_ctx.debug_rell(X, nd, 2000, seed=21, path=2)
    assert g["Y"].tobytes() == a["Y"].tobytes()                                     # LDS path bits = global path bits


def test_argument_checks_with_a_context(gpu_ctx):
    for bad in (np.zeros((1, 10)), np.zeros((65, 10))):
        with pytest.raises(engine.PmlError) as ei:
            gpu_ctx.rell_tests(bad)
        assert ei.value.code == -1
    with pytest.raises(engine.PmlError) as ei:
        gpu_ctx.rell_tests(np.zeros((2, 10)), reps=1 << 29)                          # K B >= 2^32
    assert ei.value.code == -1
    with pytest.raises(engine.PmlError) as ei:
        gpu_ctx.rell_tests(np.zeros((2, 10)), scales=[0.5, -1.0])
    assert ei.value.code == -1


def test_argument_checks_raw_abi_with_a_context(gpu_ctx):
    """the C entry points with a LIVE context: T = 1, T = 65, N >= 2^31 (the check in front of the (int) narrowing that feeds device
    indexing) and NULL pointers are PML_EINVAL; the shape is checked before anything is read, so the 8-double buffer is never touched"""
    import ctypes as C
    from pepr_amd import _lib
    L, ctx = gpu_ctx.L, gpu_ctx.ptr
    x = np.zeros(8)
    xp = x.ctypes.data_as(C.POINTER(C.c_double))
    res = _lib.TreeTestResult()
    lp = C.POINTER(C.c_longlong)
    for N, T in ((4, 1), (4, 65), (1 << 31, 2), ((1 << 31) + 5, 2), (1 << 40, 2), (0, 2), (-3, 2)):
        assert L.pml_rell_tests(ctx, N, T, xp, None, C.byref(res)) == -1, (N, T)
        assert res.ntrees == 0 and not res.au
    assert L.pml_rell_tests(ctx, 4, 2, None, None, C.byref(res)) == -1                 # NULL table
    assert L.pml_rell_tests(ctx, 4, 2, xp, None, None) == -1                           # NULL result
    nd = (C.c_longlong * 1)(4)
    bp, kh, sh = (np.zeros(4, dtype=np.int64) for _ in range(3))
    b, k, s_ = (a.ctypes.data_as(lp) for a in (bp, kh, sh))

    def dbg(N=4, T=2, tab=xp, K=1, ndp=nd, B=1, path=0, bpp=b, khp=k, shp=s_):
        return L.pml_debug_rell(ctx, N, T, tab, K, ndp, B, 0, path, None, bpp, khp, shp, None, None)
    assert dbg() == 0                                                                   # the valid call the bad ones are variations of
    assert int(bp[:2].sum()) == 1
    for kw in (dict(T=1), dict(T=65), dict(N=1 << 31), dict(N=1 << 33), dict(tab=None), dict(ndp=None), dict(bpp=None), dict(khp=None),
               dict(shp=None), dict(K=0), dict(B=0), dict(path=3), dict(K=1, B=1 << 32)):
        assert dbg(**kw) == -1, kw
    nd[0] = 0
    assert dbg() == -1                                                                  # n_k < 1
    nd[0] = 1 << 31
    assert dbg() == -1                                                                  # n_k >= 2^31
    # pml_tree_tests: T out of range, NULL alignment / trees / result
    import ctypes
    names = (ctypes.c_char_p * 3)(b"a", b"b", b"c")
    rows = (ctypes.c_char_p * 3)(b"AR", b"AR", b"AQ")
    aln = _lib.Alignment(3, 2, names, rows)
    nws = (ctypes.c_char_p * 2)(b"(a,b,c);", b"(a,b,c);")
    assert L.pml_tree_tests(ctx, None, 2, nws, None, None, None, C.byref(res), None) == -1
    assert L.pml_tree_tests(ctx, C.byref(aln), 2, None, None, None, None, C.byref(res), None) == -1
    assert L.pml_tree_tests(ctx, C.byref(aln), 2, nws, None, None, None, None, None) == -1
    assert L.pml_tree_tests(ctx, C.byref(aln), 1, nws, None, None, None, C.byref(res), None) == -1
    assert L.pml_tree_tests(ctx, C.byref(aln), 65, nws, None, None, None, C.byref(res), None) == -1
    nws[1] = None
    assert L.pml_tree_tests(ctx, C.byref(aln), 2, nws, None, None, None, C.byref(res), None) == -1


def test_meaning_on_the_synthetic_table(gpu_ctx):
    X = rell_ref.synthetic_table()
    B = 2000
    got = gpu_ctx.rell_tests(X, reps=B, seed=11)
    ref = rell_ref.tests(X, B, 11)
    best, dup, hopeless = 0, 3, 4
    assert got["sh_count"][best] == B and got["kh_count"][best] == B
    assert np.all(got["bp_count"][:, dup] == 0) and got["sh_count"][dup] == B       # ties go to the lowest index
    assert np.all(got["bp_count"][:, hopeless] == 0) and got["kh_count"][hopeless] == 0 and got["sh_count"][hopeless] == 0
    assert got["au"][hopeless] == 0.0
    print("au", got["au"], "reference", ref["au"])
    assert np.abs(got["au"][:3] - ref["au"][:3]).max() <= 3e-13                     # the host-test tolerance
    assert list(got["rank"]) == [1, 3, 4, 2, 5]


def _nni_neighbours(newick):
    """the two NNI rearrangements around the first internal edge below the root: ((A,B),C,...) -> ((A,C),B,...), ((C,B),A,...)"""
    kids, _, _ = util.parse_newick(newick)

    def fmt(n):
        k, name, ln = n
        return ("(" + ",".join(fmt(c) for c in k) + ")" if k else name) + ":%.10f" % ln
    i = next(j for j, c in enumerate(kids) if len(c[0]) == 2)
    inner = kids[i]
    rest = [c for j, c in enumerate(kids) if j != i]
    A, B = inner[0]
    C = rest[0]
    out = []
    for x, y in ((A, B), (B, A)):           # C takes the place of y
        new_inner = ([x, C], "", inner[2])
        top = [new_inner, y] + rest[1:]
        out.append("(" + ",".join(fmt(c) for c in top) + ");")
    return out


def test_end_to_end_tree_tests(gpu_ctx):
    names, rows, _ = synth.simulate_alignment(10, 600, 4242)
    gene = (names, rows)
    ml = gpu_ctx.search([gene], None, spr_radius=5)[0]["newick"]
    rnd = synth.random_tree(10, np.random.default_rng(99), names)[0]
    trees = [ml, ml] + _nni_neighbours(ml) + [rnd]
    # three different arrangements of one edge (pml_rf_distance counts the splits of one tree the other lacks: 1 per NNI)
    assert engine.rf_distance(trees[2], ml) == 1 and engine.rf_distance(trees[3], ml) == 1 and engine.rf_distance(trees[2], trees[3]) == 1
    B = 2000
    got = gpu_ctx.tree_tests(gene, trees, reps=B, seed=5)
    site = got["site_lnl"]
    assert site.shape == (5, 600)
    ref = rell_ref.tests(site, B, 5)                                                # the returned values, resampled by the reference
    assert np.array_equal(got["bp_count"], ref["bp_count"])
    assert np.array_equal(got["kh_count"], ref["kh_count"]) and np.array_equal(got["sh_count"], ref["sh_count"])
    assert np.abs(got["au"] - ref["au"]).max() <= 3e-13
    assert np.abs(site.sum(axis=1) - got["lnl"]).max() <= 1e-9 * np.abs(got["lnl"]).max()
    for t, nw in enumerate(trees):
        alone = gpu_ctx.optimize([gene], [nw])[0]
        assert alone["lnl"] == got["lnl"][t], (t, alone["lnl"], got["lnl"][t])     # bit for bit: composition independence
    assert np.array_equal(site[0], site[1])
    assert got["sh_count"][4] == 0 and got["kh_count"][4] == 0 and np.all(got["bp_count"][:, 4] == 0)   # the random tree
    assert got["sh"][0] == 1.0                                                      # the ML tree
    # trees scored as given (no optimisation): the per-site values of pml_score
    asis = gpu_ctx.tree_tests(gene, trees[:2] + [rnd], optimize=False, reps=257, seed=1)
    sc = gpu_ctx.score([gene], [rnd], site_lnl=True)[0]
    assert np.array_equal(asis["site_lnl"][2], sc["site_lnl"]) and asis["lnl"][2] == sc["lnl"]


def test_runconsel_mirror(gpu_ctx):
    names, rows, true_nw = synth.simulate_alignment(8, 300, 77)
    rnd = synth.random_tree(8, np.random.default_rng(5), names)[0]
    trees = [rnd, true_nw, true_nw]
    tc = tb.TreeComparison(gpu_ctx, reps=2000, seed=3)
    lines = tc.runConsel(tb.SequenceAlignment(names, rows), trees, "8", "PROTGAMMAWAG")
    head = [l for l in lines if "rank" in l]
    assert len(head) == 1 and head[0].split() == "# rank item obs au np | bp pp kh sh |".split()
    body = lines[lines.index(head[0]) + 1:]
    assert len(body) == len(trees)
    rowre = re.compile(r"^#\s+(\d+)\s+(\d+)\s+(-?[\d.]+)\s+([\d.]+)\s+([\d.]+) \|\s+([\d.]+)\s+([\d.]+)\s+([\d.]+)\s+([\d.]+) \|$")
    parsed = [rowre.match(l).groups() for l in body]
    assert [int(p[0]) for p in parsed] == [1, 2, 3]                                 # sorted by rank
    assert [int(p[1]) for p in parsed] == [2, 3, 1]                                 # the true tree, its copy, the random tree
    assert float(parsed[2][3]) == 0.0 and float(parsed[0][8]) == 1.0                # random tree: AU 0; best tree: SH 1
    for p in parsed:
        assert all(0.0 <= float(v) <= 1.0 for v in p[3:])
