"""k_reduce, k_g20, k_sh and k_gather driven on their own (tests/kernel_harness) against their definitions (tests/kref.py)."""
import math

import numpy as np
import pytest

import kh
import kref

pytestmark = pytest.mark.gpu


def _reduce_req(dev, pat, w, out, k):
    r = kh.ReduceReq()
    r.patlnl = pat.data_ptr(); r.weight = w.data_ptr(); r.out = out.data_ptr() + 8 * k; r.mpad = pat.numel(); r.pad = 0
    return r


def test_k_reduce_against_fsum_and_reproducible():
    dev = kh.Dev()
    rng = np.random.default_rng(3)
    data = []
    for mpad in (32, 8192, 100032):
        w = rng.integers(0, 6, mpad).astype(float)
        w[rng.random(mpad) < 0.2] = 0.0
        w[-7:] = 0.0                                             # padding columns
        lnl = -rng.random(mpad) * 60 - 1
        off = np.flatnonzero(w == 0)
        lnl[off[::3]] = np.nan; lnl[off[1::3]] = -np.inf         # whatever padding holds must not reach the sum (the w != 0 guard)
        data.append((dev.put(lnl), dev.put(w), lnl, w))
    out = dev.zeros(8)
    dev.reduce([_reduce_req(dev, p, w, out, k) for k, (p, w, _, _) in enumerate(data)])
    first = out.cpu().numpy().copy()
    for k, (_, _, lnl, w) in enumerate(data):
        on = w != 0
        ref = math.fsum((w[on] * lnl[on]).tolist())
        cond = float(np.abs(w[on] * lnl[on]).sum())
        # a thread adds mpad / 256 terms in sequence, then 6 + 2 tree levels; each addition rounds at most 2^-53 of the running sum
        tol = cond * 2.0 ** -53 * (len(w) / 256 + 16)
        err = abs(first[k] - ref)
        print("KERR k_reduce mpad=%d |sum - fsum| %.3e (bound from the condition number %.3e)" % (len(w), err, tol))
        assert err <= tol, ("k_reduce", len(w), first[k], ref)
    # same bits alone, again, and in other company
    out2 = dev.zeros(8)
    dev.reduce([_reduce_req(dev, data[1][0], data[1][1], out2, 5)])
    dev.reduce([_reduce_req(dev, data[2][0], data[2][1], out2, 0), _reduce_req(dev, data[1][0], data[1][1], out2, 1),
                _reduce_req(dev, data[0][0], data[0][1], out2, 2), _reduce_req(dev, data[1][0], data[1][1], out2, 3)])
    o2 = out2.cpu().numpy()
    assert o2[5].tobytes() == first[1].tobytes() == o2[1].tobytes() == o2[3].tobytes(), "k_reduce is not reproducible"
    assert o2[0].tobytes() == first[2].tobytes() and o2[2].tobytes() == first[0].tobytes()


def test_k_g20_mixture_with_unequal_counts():
    dev = kh.Dev()
    rng = np.random.default_rng(8)
    reqs, refs = [], []
    for mpad, npat in ((32, 32), (96, 70), (4128, 4100)):
        table = 10.0 ** (-30 * rng.random((20, mpad)))
        cnt = rng.integers(0, 3, (5, mpad)).astype(np.int32)             # the five traversals were rescued differently
        cnt[:, ::7] = cnt[0, ::7]                                        # ... and sometimes alike
        weight = rng.integers(1, 4, mpad).astype(float)
        weight[npat:] = 0.0; weight[3::11] = 0.0
        table[:, npat:] = np.nan
        w = rng.random(20); w /= w.sum()
        d = dict(table=dev.put(table), cnt=dev.put(cnt), weight=dev.put(weight), out=dev.zeros(1), pat=dev.zeros(mpad))
        r = kh.G20Req()
        r.table = d["table"].data_ptr(); r.cnt = d["cnt"].data_ptr(); r.weight = d["weight"].data_ptr(); r.w[:] = w.tolist()
        r.out = d["out"].data_ptr(); r.patlnl = d["pat"].data_ptr() if mpad != 32 else None; r.mpad = mpad; r.pad = 0
        reqs.append(r)
        refs.append((d, kref.g20(np.nan_to_num(table), cnt, weight, w), weight))
    dev.g20(reqs)
    for r, (d, (lnl, pat), weight) in zip(reqs, refs):
        got = float(d["out"].cpu().numpy()[0])
        scale = float((weight * np.abs(pat.astype(float))).sum())
        err = abs(got - float(lnl)) / scale
        print("KERR k_g20 mpad=%d |lnL - ref| / sum w |lnL_p| %.3e (pinned %.1e, ceiling 1e-10)" % (r.mpad, err, TOL_G20))
        assert err <= TOL_G20, ("k_g20 lnL", r.mpad, got, float(lnl))
        if r.patlnl:
            perr = float(np.abs(d["pat"].cpu().numpy() - pat.astype(float)).max())
            print("KERR k_g20 mpad=%d per-pattern lnL max error %.3e (pinned %.1e, ceiling 1e-11)" % (r.mpad, perr, TOL_G20_PAT))
            assert perr <= TOL_G20_PAT, ("k_g20 per-pattern lnL", r.mpad, perr)


TOL_G20, TOL_G20_PAT = 1.2e-15, 4.6e-13        # 8 x observed (1.4e-16, 5.7e-14); ceilings 1e-10, 1e-11


def test_k_sh_resampling_counts_exactly():
    """per-pattern values are multiples of 2^-20, so every sum is exact whatever its order: the support must match to the bit"""
    dev = kh.Dev()
    rng = np.random.default_rng(21)
    reqs, npats, want, outs = [], [], [], []
    for nsites, npat, nboot, seed, lead in ((100, 37, 1, 5, 40), (100, 37, 100, 5, 40), (257, 64, 1000, 123456789012345, 25), (64, 20, 100, 0, -30)):
        l = [-(rng.integers(1 << 18, 1 << 24, npat)) / float(1 << 20) for _ in range(3)]
        s2p = rng.integers(0, npat, nsites).astype(np.int32)
        l[0] = l[0] + lead / 64.0                                        # an observed advantage of the size of a resample's scatter
        ts = [dev.put(x) for x in l]
        m = dev.put(s2p); out = dev.zeros(1)
        r = kh.ShReq()
        r.l0, r.l1, r.l2 = (t.data_ptr() for t in ts)
        r.site2pat = m.data_ptr(); r.out = out.data_ptr(); r.seed = seed; r.nsites = nsites; r.nboot = nboot
        reqs.append(r); npats.append(npat); outs.append(out)
        want.append(kref.sh_support(l[0], l[1], l[2], s2p, seed, nboot)[0])
    dev.sh(reqs, npats)
    got = [float(o.cpu().numpy()[0]) for o in outs]
    print("KERR k_sh supports", got, "reference", want)
    assert got == want, ("k_sh", got, want)
    assert any(0.0 < g < 1.0 for g in got), "no case exercises both outcomes of a resample"


def test_k_gather_copies_exactly():
    dev = kh.Dev()
    rng = np.random.default_rng(13)
    ntax_dst, dst_mpad = 6, 160
    dst0 = np.full((ntax_dst, dst_mpad), 99, np.uint8); w0 = np.full(dst_mpad, -1.0)
    dst, dst_w = dev.put(dst0), dev.put(w0)
    segs, rows, want, want_w = [], [], dst0.copy(), w0.copy()
    for nrow, src_mpad, npat, off, rowmap in ((5, 64, 50, 7, [4, -1, 0, 2, -1, 1]), (3, 96, 96, 57, [-1, 2, 2, 0, 1, -1]), (2, 32, 1, 159, [1, 0, -1, -1, 1, 0])):
        src = rng.integers(0, 23, (nrow, src_mpad)).astype(np.uint8)
        w = rng.integers(1, 9, npat).astype(float)
        g = kh.GatherSeg()
        g.src = dev.put(src).data_ptr(); g.w = dev.put(w).data_ptr(); g.dst = dst.data_ptr(); g.dst_w = dst_w.data_ptr()
        g.rowmap = dev.put(np.array(rowmap, np.int32)).data_ptr()
        g.src_mpad = src_mpad; g.npat = npat; g.dst_mpad = dst_mpad; g.dst_off = off; g.ntax_dst = ntax_dst; g.pad = 0
        segs.append(g); rows.append(nrow)
        kref.gather(want, want_w, src, w, rowmap, npat, off)
    dev.gather(segs, rows)
    assert np.array_equal(dst.cpu().numpy(), want), "k_gather codes"
    assert np.array_equal(dst_w.cpu().numpy(), want_w), "k_gather weights"
    assert (want == 99).any() and (want == 22).any()                     # untouched columns and gap rows both occur
