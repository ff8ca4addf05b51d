"""k_oplist driven on its own (variants 1 and 11 through launch_oplist, tests/kernel_harness): every ordered pair of side kinds as
a newview and as a sumtable, the evaluate tails, register chaining with unstored results, and the 2^256 rescue, against the
longdouble references of tests/kref.py on the matrices k_pmat produced.  Results are compared as TRUE values, stored entry x 2^(-256 count)."""
import numpy as np
import pytest

import kh
import kref
from pepr_amd import synth

pytestmark = pytest.mark.gpu
LD = np.longdouble
KINDS = (kh.SK_CLV, kh.SK_TIP, kh.SK_CHERRY, kh.SK_PITCH)
NAMES = {kh.SK_CLV: "CLV", kh.SK_TIP: "TIP", kh.SK_CHERRY: "CHERRY", kh.SK_PITCH: "PITCH"}
# relative to the pattern's largest entry / absolute per-pattern lnL: pinned, ceiling
TOL_CLV, CEIL_CLV = 1.2e-14, 1e-12        # observed 1.5e-15
TOL_LNL, CEIL_LNL = 9.1e-13, 1e-11        # observed 1.1e-13 (one ulp of a per-pattern lnL of several hundred)
LENS = dict(l=0.07, r=0.31, a=0.11, b=0.23, c=0.05, inner=0.4, ev=0.13)


class World:
    """one gene: model, branch matrices from k_pmat (tested on its own) beside the exact ones, tip codes, two input CLVs with counts"""

    def __init__(self, mpad, seed, chained):
        self.dev = dev = kh.Dev()
        self.mpad, self.npat, self.chained = mpad, mpad - 3, chained
        rng = np.random.default_rng(seed)
        _, _, pi3 = synth.wag_constants()
        ms, self.eig = kh.model_struct(pi3)
        self.pi = pi3
        self.model = dev.struct(ms)
        self.rates = kref.gamma_rates(0.8)
        names = list(LENS)
        reqs = []
        for n in names:
            for kind in (kh.PM_FRAGS, kh.PM_FRAGS_PI, kh.PM_TIPTABLE):
                r = kh.PmatReq(); r.t = LENS[n]; r.rates[:] = list(self.rates); r.kind = kind
                reqs.append(r)
        arr = (kh.PmatReq * len(reqs))(*reqs)
        self.frags = dev.zeros(len(reqs) * kh.FRAG_STRIDE)
        dev._call(kh.lib().kh_pmat, self.model.data_ptr(), arr, len(reqs), 0, dev.desc.data_ptr(), self.frags.data_ptr(), dev.stream)
        self.slot = {(n, kind): self.frags.data_ptr() + 8 * kh.FRAG_STRIDE * (3 * i + kind) for i, n in enumerate(names) for kind in range(3)}
        # the reference contracts the SAME matrices the kernel is given (k_pmat's, held to expm in test_gpu_kernel_pmat.py): with
        # the exact ones the comparison measures P's 4e-15 absolute error, which is 5e-12 of a pattern whose entries are all
        # products of small off-diagonal elements (observed; DESIGN.md "Kernel-level error budget")
        host = self.frags.cpu().numpy().reshape(len(reqs), kh.FRAG_STRIDE)
        self.P = {n: kh.frag_unpack(host[3 * i]).astype(LD) for i, n in enumerate(names)}
        self.eigf = dev.eigfrags(self.model, 1)
        self.codes = {k: rng.integers(0, 23, self.npat) for k in "abcdefg"}
        self.d_codes = {k: dev.codes(v, mpad) for k, v in self.codes.items()}
        self.clv, self.cnt, self.d_clv, self.d_cnt = {}, {}, {}, {}
        for k in "AB":
            v = rng.random((4, 20, self.npat)) * 10.0 ** (-70 * rng.random(self.npat))[None, None, :]
            self.set_clv(k, v, rng.integers(0, 3, self.npat))

    def set_clv(self, k, v, cnt):
        self.clv[k], self.cnt[k] = v, np.asarray(cnt)
        self.d_clv[k] = self.dev.put(kh.clv_pack(v.reshape(80, -1), self.mpad))
        full = np.zeros(self.mpad, np.int32); full[:self.npat] = cnt
        self.d_cnt[k] = self.dev.put(full)

    # a side: (kind, descriptor fields, counts pointer, fragment-set name, true-scale operand of the reference)
    def side(self, kind, which):
        s = kh.OpSide()
        if kind == kh.SK_CLV:
            k = "A" if which == "l" else "B"
            s.p0 = self.d_clv[k].data_ptr()
            return s, self.d_cnt[k].data_ptr(), kref.true_clv(self.clv[k], self.cnt[k])
        tips = "abc" if which == "l" else "def"
        s.p0 = self.d_codes[tips[0]].data_ptr()
        if kind == kh.SK_TIP:
            return s, None, kref.tip_operand(self.codes[tips[0]])
        s.p1 = self.d_codes[tips[1]].data_ptr()
        s.t0, s.t1 = self.slot[("a", 2)], self.slot[("b", 2)]
        if kind == kh.SK_CHERRY:
            return s, None, kref.cherry_operand(self.P["a"], self.codes[tips[0]], self.P["b"], self.codes[tips[1]])
        s.p2 = self.d_codes[tips[2]].data_ptr(); s.t2 = self.slot[("c", 2)]; s.f = self.slot[("inner", 0)]
        return s, None, kref.pitch_operand(self.P["a"], self.codes[tips[0]], self.P["b"], self.codes[tips[1]], self.P["inner"], self.P["c"], self.codes[tips[2]])

    def op(self, mode, lk, rk, flags=0, chain_from=None):
        """-> (descriptor, output tensors, reference of the TRUE result); chain_from: true-scale operand that sits in the registers"""
        o = kh.NvOp()
        o.l, o.l_scl, L = self.side(lk, "l")
        o.r, o.r_scl, R = self.side(rk, "r")
        if chain_from is not None:
            L = chain_from; o.l = kh.OpSide(); o.l_scl = None; flags |= kh.OPF_CHAIN_L
        o.mpad = self.mpad; o.flags = lk | (rk << 2) | flags; o.mode = mode
        dev = self.dev
        if mode == kh.MODE_NEWVIEW:
            o.pl, o.pr = self.slot[("l", 0)], self.slot[("r", 0)]
            out, scl = dev.put(np.full(kh.clv_doubles(self.mpad), -7.0)), dev.put(np.full(self.mpad, -7, np.int32))
            ref = kref.newview(self.P["l"], L, self.P["r"], R)
        elif mode == kh.MODE_SUMTABLE:
            o.pl = self.eigf.data_ptr(); o.pr = self.eigf.data_ptr() + 8 * kh.PFRAG
            out, scl = dev.put(np.full(kh.clv_doubles(self.mpad), -7.0)), dev.put(np.full(self.mpad, -7, np.int32))
            ref = kref.sumtable(self.eig, L, R)
        elif mode == kh.MODE_EVALUATE:
            o.pl = o.pr = self.slot[("ev", 1)]
            out, scl = dev.put(np.full(self.mpad, -7.0)), None
            ref = kref.evaluate(self.pi, self.P["ev"], L, R)
        else:
            o.pl = o.pr = self.slot[("ev", 1)]
            out, scl = dev.put(np.full(4 * self.mpad, -7.0)), dev.put(np.full(self.mpad, -7, np.int32))
            ref = kref.evaluate_cat(self.pi, self.P["ev"], L, R)
        o.out = out.data_ptr(); o.out_scl = scl.data_ptr() if scl is not None else None
        return o, (out, scl), ref

    def compare(self, mode, outs, ref, what):
        """-> (observed error, counts read back)"""
        out, scl = outs
        n = self.npat
        cnt = scl.cpu().numpy()[:n] if scl is not None else None
        if mode in (kh.MODE_NEWVIEW, kh.MODE_SUMTABLE):
            got = kref.true_clv(kh.clv_unpack(out.cpu().numpy(), self.mpad)[:, :n].reshape(4, 20, n), cnt)
            big = np.abs(ref).max(axis=(0, 1))
            err = float((np.abs(got - ref).max(axis=(0, 1))[big > 0] / big[big > 0]).max())
            assert np.all(got[:, :, big == 0] == 0), what
            assert err <= TOL_CLV, ("k_oplist " + what, err)
        elif mode == kh.MODE_EVALUATE:
            err = float(np.abs(out.cpu().numpy()[:n] - ref.astype(float)).max())
            assert err <= TOL_LNL, ("k_oplist " + what, err)
        else:
            got = np.ldexp(out.cpu().numpy().reshape(4, self.mpad)[:, :n].astype(LD), (-256 * cnt.astype(np.int64))[None, :].astype(np.int32))
            err = float((np.abs(got - ref) / ref.max(0)[None, :]).max())
            assert err <= TOL_CLV, ("k_oplist " + what, err)
        return err, cnt


def rescue_rule(w, ref, lcnt, rcnt):
    """the oracle's rule (pml_oracle.c: a pattern whose largest STORED entry is below 2^-256 is multiplied by 2^256, once): the
    count a result must carry, and which patterns sit too close to the threshold for the rule to be decidable in double"""
    base = lcnt + rcnt
    stored_max = np.ldexp(np.abs(ref).max(axis=(0, 1)), (256 * base).astype(np.int32))
    thr = np.ldexp(LD(1), -256)
    return base + (stored_max < thr), np.abs(stored_max / thr - 1) < 1e-9


@pytest.mark.parametrize("chained", [False, True], ids=["variant1", "variant11"])
@pytest.mark.parametrize("mpad", [32, 160, 4128])
def test_k_oplist_every_pair_of_side_kinds(mpad, chained):
    """16 newviews and 16 sumtables, one run each, in one launch (three mpads over the parametrisation; padding columns npat..mpad)"""
    w = World(mpad, 7 + mpad, chained)
    ops, outs, meta = [], [], []
    for mode in (kh.MODE_NEWVIEW, kh.MODE_SUMTABLE):
        for lk in KINDS:
            for rk in KINDS:
                o, out, ref = w.op(mode, lk, rk, flags=kh.OPF_NT_STORE if (mode == kh.MODE_NEWVIEW and (lk + rk) % 2) else 0)
                ops.append(o); outs.append(out); meta.append((mode, lk, rk, ref))
    w.dev.oplist(ops, [(i, i + 1) for i in range(len(ops))], chained)
    worst = {}
    for out, (mode, lk, rk, ref) in zip(outs, meta):
        name = "%s %s x %s mpad=%d" % ("newview" if mode == kh.MODE_NEWVIEW else "sumtable", NAMES[lk], NAMES[rk], mpad)
        err, cnt = w.compare(mode, out, ref, name)
        lc = w.cnt["A"] if lk == kh.SK_CLV else 0 * w.cnt["A"]
        rc = w.cnt["B"] if rk == kh.SK_CLV else 0 * w.cnt["B"]
        if mode == kh.MODE_NEWVIEW:
            want, close = rescue_rule(w, ref, lc, rc)
            assert np.array_equal(cnt[~close], want[~close]), ("k_oplist rescue count " + name, cnt, want)
        else:
            assert np.array_equal(cnt, lc + rc), ("k_oplist sumtable count " + name)
        key = "newview" if mode == kh.MODE_NEWVIEW else "sumtable"
        worst[key] = max(worst.get(key, 0.0), err)
    for k, e in worst.items():
        print("KERR k_oplist %s all side pairs mpad=%d %s max error / largest entry %.3e (pinned %.1e, ceiling %.0e)"
              % (k, mpad, "variant 11" if chained else "variant 1", e, TOL_CLV, CEIL_CLV))


@pytest.mark.parametrize("chained", [False, True], ids=["variant1", "variant11"])
def test_k_oplist_evaluate_tails(chained):
    w = World(160, 3, chained)
    ops, outs, meta = [], [], []
    for mode in (kh.MODE_EVALUATE, kh.MODE_EVALUATE_CAT):
        for lk, rk in ((kh.SK_CLV, kh.SK_TIP), (kh.SK_TIP, kh.SK_CLV), (kh.SK_CLV, kh.SK_CLV), (kh.SK_CHERRY, kh.SK_CHERRY), (kh.SK_PITCH, kh.SK_CLV), (kh.SK_CLV, kh.SK_CHERRY)):
            o, out, ref = w.op(mode, lk, rk)
            ops.append(o); outs.append(out); meta.append((mode, lk, rk, ref))
    w.dev.oplist(ops, [(i, i + 1) for i in range(len(ops))], chained)
    for out, (mode, lk, rk, ref) in zip(outs, meta):
        name = "%s %s x %s" % ("evaluate" if mode == kh.MODE_EVALUATE else "evaluate-cat", NAMES[lk], NAMES[rk])
        err, cnt = w.compare(mode, out, ref, name)
        print("KERR k_oplist %s %s error %.3e" % (name, "variant 11" if chained else "variant 1", err))
        if cnt is not None:
            assert np.array_equal(cnt, w.cnt["A"] * (lk == kh.SK_CLV) + w.cnt["B"] * (rk == kh.SK_CLV)), name


def _underflowing_world(chained):
    """input A rescaled column by column by exact powers of two so that chosen patterns of newview(A, B) end just below 2^-256
    (rescued), just above it (not rescued), or are impossible (all zero): lanes .x only, .y only, both, and two waves of a tile"""
    w = World(160, 5, chained)
    _, _, L = w.side(kh.SK_CLV, "l"); _, _, R = w.side(kh.SK_CLV, "r")
    ref = kref.newview(w.P["l"], L, w.P["r"], R)
    stored = np.ldexp(np.abs(ref).max(axis=(0, 1)), (256 * (w.cnt["A"] + w.cnt["B"])).astype(np.int32))
    e = np.floor(np.log2(stored)).astype(int)
    A = w.clv["A"].copy()
    below, above, zero = [0, 3, 4, 5, 40, 41, 100], [1, 6, 7, 42, 101], [9, 70]
    for p in below:
        A[:, :, p] = np.ldexp(A[:, :, p], -257 - e[p])
    for p in above:
        A[:, :, p] = np.ldexp(A[:, :, p], -256 - e[p])
    A[:, :, zero] = 0.0
    cnt = w.cnt["A"].copy(); cnt[below[:3]] = 1
    cb = w.cnt["B"].copy(); cb[below[:3]] = 2                       # 1 + 2, to which the rescue adds its own
    w.set_clv("A", A, cnt); w.set_clv("B", w.clv["B"], cb)
    return w, below, above, zero


@pytest.mark.parametrize("chained", [False, True], ids=["variant1", "variant11"])
def test_k_oplist_rescue_stored(chained):
    w, below, above, zero = _underflowing_world(chained)
    o, out, ref = w.op(kh.MODE_NEWVIEW, kh.SK_CLV, kh.SK_CLV)
    w.dev.oplist([o], [(0, 1)], chained)
    err, cnt = w.compare(kh.MODE_NEWVIEW, out, ref, "rescue newview CLV x CLV")
    want, close = rescue_rule(w, ref, w.cnt["A"], w.cnt["B"])
    assert not close.any()
    base = w.cnt["A"] + w.cnt["B"]
    assert np.all(want[below + zero] == base[below + zero] + 1) and np.all(want[above] == base[above])      # the construction holds
    assert np.array_equal(cnt, want), ("k_oplist rescue count", cnt[below], want[below], cnt[above], want[above])
    print("KERR k_oplist rescue stored %s error %.3e; counts equal the oracle's rule on %d rescued patterns" % ("variant 11" if chained else "variant 1", err, int((want > base).sum())))


def test_k_oplist_chain_with_unstored_results_and_rescue_in_registers():
    """four dependent operations of one gene: newview (rescued patterns, OPF_NO_STORE) -> newview (OPF_CHAIN_L, OPF_NO_STORE) ->
    newview (OPF_CHAIN_L, stored) -> evaluate (OPF_CHAIN_L); and the same head into a sumtable tail in a second run"""
    w, below, above, zero = _underflowing_world(True)
    runs, ops, checks = [], [], []
    for tail in (kh.MODE_EVALUATE, kh.MODE_SUMTABLE):
        b = len(ops)
        o0, out0, r0 = w.op(kh.MODE_NEWVIEW, kh.SK_CLV, kh.SK_CLV, flags=kh.OPF_NO_STORE)
        o1, out1, r1 = w.op(kh.MODE_NEWVIEW, kh.SK_CLV, kh.SK_CHERRY, flags=kh.OPF_NO_STORE, chain_from=r0)
        o2, out2, r2 = w.op(kh.MODE_NEWVIEW, kh.SK_CLV, kh.SK_TIP, flags=kh.OPF_NT_STORE, chain_from=r1)
        o3, out3, r3 = w.op(tail, kh.SK_CLV, kh.SK_CLV if tail == kh.MODE_SUMTABLE else kh.SK_TIP, chain_from=r2)
        ops += [o0, o1, o2, o3]; runs.append((b, b + 4))
        checks += [(kh.MODE_NEWVIEW, out2, r2, "chained newview (third of four)"), (tail, out3, r3, "chained tail mode %d" % tail)]
        unstored = (out0, out1)
    w.dev.oplist(ops, runs, True)
    for mode, out, ref, name in checks:
        big = np.abs(ref).max(axis=(0, 1)) if mode != kh.MODE_EVALUATE else None
        if mode == kh.MODE_EVALUATE:
            live = np.isfinite(ref.astype(float))                # impossible patterns (all-zero input) have lnL = -inf on both sides
            got = out[0].cpu().numpy()[:w.npat]
            assert np.all(np.isneginf(got[~live])), name
            err = float(np.abs(got[live] - ref[live].astype(float)).max())
            assert err <= TOL_LNL, ("k_oplist " + name, err)
        else:
            err, _ = w.compare(mode, out, ref, name)
        print("KERR k_oplist %s error %.3e" % (name, err))
    for out, scl in unstored:                                    # OPF_NO_STORE: nothing was written
        assert np.all(out.cpu().numpy() == -7.0) and np.all(scl.cpu().numpy() == -7)
