"""Plain high-precision references of the operations the device kernels perform, written from the mathematics:

* Q from tests/golden/wag_constants.json (S, pi) and P(t r) = expm(Q t r) by mpmath at 50 digits: p_expm is mpmath.expm itself,
  p_exact (used in bulk: 30 x faster) the spectral form in the same 50-digit arithmetic, held to p_expm by the CPU tests --
  never the double-precision eigensystem the kernels are given;
* discrete-Gamma mean rates from mpmath's incomplete gamma function;
* newview / evaluate / sumtable in numpy.longdouble on the exact P, with the TRUE value of every entry (a stored entry times
  2^(-256 count): exact in longdouble, whose exponent range covers 60 rescues) instead of 2^256 steps;
* Newton's f, f', f'' from their definition, exp(lambda r t) by mpmath, summed in longdouble;
* the Gamma20 mixture, the SH resampling hash and the replicate gather from their definitions in kernels.h.

Nothing here looks at oracle/ or at the kernels' order of operations."""
import functools
import math

import mpmath as mp
import numpy as np

from pepr_amd import synth

mp.mp.dps = 50
LD = np.longdouble
NS, NCAT, NCODES = 20, 4, 23


def _ld(x):
    """mpmath number -> longdouble (two-step: leading double + remainder)"""
    hi = float(x)
    return LD(hi) + LD(float(x - mp.mpf(hi)))


def q_mp(pi):
    """WAG rate matrix for frequencies pi, normalised to one expected substitution per unit time (mpmath matrix)"""
    S, _, _ = synth.wag_constants()
    pi = [mp.mpf(float(x)) for x in pi]
    tot = mp.fsum(pi)
    pi = [x / tot for x in pi]
    Q = mp.zeros(NS, NS)
    for i in range(NS):
        for j in range(NS):
            if i != j:
                Q[i, j] = mp.mpf(float(S[i, j])) * pi[j]
        Q[i, i] = -mp.fsum(Q[i, j] for j in range(NS) if j != i)
    mu = -mp.fsum(pi[i] * Q[i, i] for i in range(NS))
    return Q / mu, pi


@functools.lru_cache(maxsize=None)
def _q_cached(pi_key):
    return q_mp(pi_key)


@functools.lru_cache(maxsize=None)
def _p_expm(pi_key, tr):
    P = mp.expm(_q_cached(pi_key)[0] * mp.mpf(tr))
    return np.array([[_ld(P[i, j]) for j in range(NS)] for i in range(NS)], LD)


def p_expm(pi, t, rate):
    """P(t rate) = expm(Q t rate) by mpmath.expm (scaling and squaring of a Taylor series) as longdouble[20][20]: the definition.
    0.3 s per matrix -- p_exact below is what the kernel tests use in bulk, pinned to this one in the CPU tests."""
    return _p_expm(tuple(float(x) for x in pi), float(t) * float(rate))


@functools.lru_cache(maxsize=None)
def _spectral(pi_key):
    """Q = D^-1/2 B D^1/2 with B symmetric: B's eigensystem at 50 digits.  The cancellation U diag(exp(lambda t)) U^-1 suffers in
    double precision at t -> 0 costs 6 of 50 digits here; tests/test_kernel_harness_cpu.py holds the result to mpmath.expm"""
    Q, pi = _q_cached(pi_key)
    sp = [mp.sqrt(x) for x in pi]
    B = mp.matrix(NS, NS)
    for i in range(NS):
        for j in range(NS):
            B[i, j] = sp[i] * Q[i, j] / sp[j]
    B = (B + B.T) / 2
    lam, V = mp.eigsy(B)
    return [lam[i] for i in range(NS)], V, sp


@functools.lru_cache(maxsize=None)
def _p_exact(pi_key, tr):
    lam, V, sp = _spectral(pi_key)
    e = [mp.e ** (l * mp.mpf(tr)) for l in lam]
    out = np.zeros((NS, NS), LD)
    for i in range(NS):
        for j in range(NS):
            out[i, j] = _ld(mp.fsum(V[i, k] * e[k] * V[j, k] for k in range(NS)) * sp[j] / sp[i])
    return out


def p_exact(pi, t, rate):
    """P(t rate) as longdouble[20][20], 50-digit arithmetic throughout; t * rate is formed in double, as the kernel's request does"""
    return _p_exact(tuple(float(x) for x in pi), float(t) * float(rate))


def p_cats(pi, t, rates):
    return np.stack([p_exact(pi, t, r) for r in rates])


@functools.lru_cache(maxsize=None)
def gamma_rates(alpha, K=4):
    """mean rates of K equal-probability categories of Gamma(shape alpha, mean 1) (Yang 1994), mpmath"""
    from scipy.special import gammaincinv
    a = mp.mpf(alpha)
    lx = [mp.findroot(lambda v, k=k: mp.gammainc(a, 0, mp.e ** v, regularized=True) - mp.mpf(k) / K, math.log(gammaincinv(alpha, k / K)))
          for k in range(1, K)]
    cdf = [mp.mpf(0)] + [mp.gammainc(a + 1, 0, mp.e ** v, regularized=True) for v in lx] + [mp.mpf(1)]
    return tuple(float((cdf[k + 1] - cdf[k]) * K) for k in range(K))


def indicators():
    ind = np.zeros((NCODES, NS), LD)
    ind[np.arange(20), np.arange(20)] = 1
    ind[20, [2, 3]] = 1; ind[21, [5, 6]] = 1; ind[22, :] = 1
    return ind


def true_clv(stored, counts):
    """stored[4][20][n] doubles with per-pattern rescue counts -> the values they stand for (longdouble)"""
    return np.ldexp(np.asarray(stored, LD), (-256 * np.asarray(counts, np.int64))[None, None, :].astype(np.int32))


def contract(P, X):
    """P[4][20][20] . X[4][20][n] per category"""
    return np.einsum("csj,cjn->csn", np.asarray(P, LD), np.asarray(X, LD))


def tip_operand(codes):
    """a tip as the operand of a contraction: 0/1 rows [4][20][n]"""
    v = indicators()[np.asarray(codes)].T
    return np.broadcast_to(v, (NCAT,) + v.shape)


def cherry_operand(P0, codes0, P1, codes1):
    return contract(P0, tip_operand(codes0)) * contract(P1, tip_operand(codes1))


def pitch_operand(P0, codes0, P1, codes1, Pin, P2, codes2):
    return contract(Pin, cherry_operand(P0, codes0, P1, codes1)) * contract(P2, tip_operand(codes2))


def newview(PL, L, PR, R):
    """true values of the parent's CLV [4][20][n]"""
    return contract(PL, L) * contract(PR, R)


def evaluate_cat(pi, P, L, R):
    """per-category likelihoods [4][n]: sum_s L_c[s] pi_s (P_c . R_c)[s]"""
    pin = np.asarray(pi, LD) / np.sum(np.asarray(pi, LD))
    return np.einsum("csn,s,csn->cn", np.asarray(L, LD), pin, contract(P, R))


def evaluate(pi, P, L, R):
    """per-pattern lnL = ln(1/4 sum_c ...)"""
    return np.log(evaluate_cat(pi, P, L, R).sum(0) / LD(4))


def sumtable(eig, L, R):
    """tab[c][i][n] = (sum_s pi_s U[s][i] L_c[s]) (sum_j Uinv[i][j] R_c[j]) for the eigensystem (lam, U, Uinv, pi) given to the kernel"""
    _, U, Uinv, pi = eig
    x = np.einsum("s,si,csn->cin", np.asarray(pi, LD), np.asarray(U, LD), np.asarray(L, LD))
    y = np.einsum("ij,cjn->cin", np.asarray(Uinv, LD), np.asarray(R, LD))
    return x * y


def newton_terms(lam, rates, t):
    """(lambda_i r_c)[4][20] and exp(lambda_i r_c t)[4][20], the products formed in double as on the device, exp by mpmath"""
    lr = np.array([[float(l) * float(r) for l in lam] for r in rates])
    ex = np.array([[_ld(mp.e ** (mp.mpf(v) * mp.mpf(float(t)))) for v in row] for row in lr], LD)
    return lr.astype(LD), ex


def newton_eval(tab, weight, counts, lam, rates, t):
    """(lnL, dlnL/dt, d2lnL/dt2, per-pattern lnL) from a sumtable of TRUE-scale or stored values tab[4][20][n] with counts"""
    lr, ex = newton_terms(lam, rates, t)
    tab = np.asarray(tab, LD)
    f = np.einsum("cin,ci->n", tab, ex)
    f1 = np.einsum("cin,ci->n", tab, ex * lr)
    f2 = np.einsum("cin,ci->n", tab, ex * lr * lr)
    w = np.asarray(weight, LD)
    on = w != 0
    pat = np.zeros(len(w), LD)
    pat[on] = np.log(f[on] / LD(4)) - np.asarray(counts, LD)[on] * LD(256) * np.log(LD(2))
    r1 = np.zeros(len(w), LD); r2 = np.zeros(len(w), LD)
    r1[on] = f1[on] / f[on]; r2[on] = f2[on] / f[on]
    return (w * pat).sum(), (w * r1).sum(), (w * (r2 - r1 * r1)).sum(), pat


def g20(table, cnt, weight, w):
    """kernels.h G20Req: lnL = sum_p weight_p ( ln sum_k w_k table[k][p] 2^(-256 cnt[k/4][p]) ), patterns of weight 0 skipped"""
    table = np.asarray(table, LD); cnt = np.asarray(cnt, np.int64)
    true = np.ldexp(table, (-256 * np.repeat(cnt, 4, axis=0)).astype(np.int32))
    s = (np.asarray(w, LD)[:, None] * true).sum(0)
    wt = np.asarray(weight, LD)
    pat = np.zeros(len(wt), LD)
    pat[wt != 0] = np.log(s[wt != 0])
    return (wt * pat).sum(), pat


M64 = (1 << 64) - 1


def mix64(z):
    z &= M64
    z ^= z >> 30; z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 27; z = (z * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def sh_columns(seed, r, nsites):
    """kernels.h ShReq: col(r, j) = mix64((seed+1) * 0x9E3779B97F4A7C15 + r * nsites + j) % nsites"""
    base = ((seed + 1) * 0x9E3779B97F4A7C15) & M64
    return [mix64(base + r * nsites + j) % nsites for j in range(nsites)]


def sh_support(l0, l1, l2, site2pat, seed, nboot):
    """fraction of resamples whose best centred arrangement leads by less than the observed advantage of l0; each sum in
    math.fsum -> (support, smallest distance of any comparison from a tie, for the caller to judge rounding)"""
    ls = [np.asarray(x, np.float64)[np.asarray(site2pat)] for x in (l0, l1, l2)]
    orig = [math.fsum(x) for x in ls]
    delta = orig[0] - max(orig[1], orig[2])
    if not delta > 0 or nboot == 0:
        return 0.0, abs(delta)
    n, hit, margin = len(site2pat), 0, abs(delta)
    for r in range(nboot):
        cols = sh_columns(seed, r, n)
        s = sorted((math.fsum(x[cols]) - o for x, o in zip(ls, orig)), reverse=True)
        hit += (s[0] - s[1]) < delta
        margin = min(margin, abs((s[0] - s[1]) - delta))
    return hit / nboot, margin


def gather(dst, dst_w, src, w, rowmap, npat, dst_off):
    """kernels.h GatherSeg: dst[t][dst_off + p] = rowmap[t] >= 0 ? src[rowmap[t]][p] : gap code, dst_w[dst_off + p] = w[p]"""
    for t, row in enumerate(rowmap):
        dst[t, dst_off:dst_off + npat] = src[row, :npat] if row >= 0 else NCODES - 1
    dst_w[dst_off:dst_off + npat] = w[:npat]
