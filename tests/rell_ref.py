"""The tree selection tests restated in numpy from their definitions (include/peprml.h, "Tree selection tests"): the
reference the device kernel and the host fit are checked against.  Nothing here is shared with the library.

  draws   site_j = ((mix64(base + ((k B + b) << 32) + j) >> 32) * N) >> 32, base = (seed + 1) * 0x9E3779B97F4A7C15 mod 2^64
  sums    Y[k][b][t] = sum_j X[t][site_j], SEQUENTIAL double additions in ascending j (np.sum adds pairwise and rounds
          differently): replicate_sums
  counts  bp / kh / sh as integers;  AU by weighted least squares with scipy's normal distribution
"""
import numpy as np

U64 = np.uint64
GOLDEN = 0x9E3779B97F4A7C15
MASK = (1 << 64) - 1


def mix64(z):
    z = z.astype(U64, copy=True)
    z ^= z >> U64(30)
    z *= U64(0xBF58476D1CE4E5B9)
    z ^= z >> U64(27)
    z *= U64(0x94D049BB133111EB)
    z ^= z >> U64(31)
    return z


def draws(seed, k, B, b, nk, N):
    """sites [len(b), nk] drawn by the replicates b of scale k"""
    base = ((seed + 1) * GOLDEN) & MASK
    with np.errstate(over="ignore"):
        key = U64(base) + ((U64(k) * U64(B) + np.asarray(b, dtype=U64)) << U64(32))
        h = mix64(key[:, None] + np.arange(nk, dtype=U64)[None, :])
        return (((h >> U64(32)) * U64(N)) >> U64(32)).astype(np.int64)


def replicate_sums(site_lnl, ndraws, B, seed, bs=None, use_cumsum=False):
    """Y[K, B, T]; site_lnl is T x N; bs = the replicates wanted (default all B).  The sums are SEQUENTIAL in the draws: draw j
    of every replicate is added, as one vector operation over the replicates, before draw j + 1 -- per replicate the same
    chain of roundings as np.cumsum(X[sites], axis=draws)[-1], which use_cumsum=True computes instead (slower: it writes every
    prefix; tests/test_tree_tests_host.py holds the two to the same bits)"""
    X = np.ascontiguousarray(np.asarray(site_lnl, dtype=np.float64).T)        # [N, T]
    N, T = X.shape
    bs = np.arange(B) if bs is None else np.asarray(bs)
    Y = np.zeros((len(ndraws), len(bs), T))
    for k, nk in enumerate(ndraws):
        nk = int(nk)
        step = max(1, (1 << 22) // max(1, nk * (T if use_cumsum else 1)))
        for lo in range(0, len(bs), step):
            s = draws(seed, k, B, bs[lo:lo + step], nk, N)                     # [chunk, nk]
            if use_cumsum:
                Y[k, lo:lo + step] = np.cumsum(X[s], axis=1)[:, -1, :]
                continue
            acc = np.zeros((s.shape[0], T))
            for col in np.ascontiguousarray(s.T):                              # draws in ascending j
                acc += X[col]
            Y[k, lo:lo + step] = acc
    return Y


def column_sums(site_lnl):
    return np.cumsum(np.asarray(site_lnl, dtype=np.float64), axis=1)[:, -1]   # L_t in site order


def k1_of(r):
    r = np.asarray(r, dtype=np.float64)
    return int(np.argmin(np.abs(r - 1.0)))                                    # the first of equals


def counts(site_lnl, ndraws, B, seed, Y=None):
    """(bp[K, T], kh[T], sh[T], k1) as integers"""
    X = np.asarray(site_lnl, dtype=np.float64)
    T, N = X.shape
    nd = np.asarray(ndraws, dtype=np.int64)
    if Y is None:
        Y = replicate_sums(X, nd, B, seed)
    K = len(nd)
    L = column_sums(X)
    bp = np.zeros((K, T), dtype=np.int64)
    for k in range(K):
        bp[k] = np.bincount(np.argmax(Y[k], axis=1), minlength=T)              # argmax: the first of equals
    k1 = k1_of(nd / float(N))
    Cc = Y[k1] * (float(N) / float(nd[k1])) - L[None, :]
    sh = np.sum((Cc.max(axis=1)[:, None] - Cc) >= (L.max() - L)[None, :], axis=0).astype(np.int64)
    kh = np.zeros(T, dtype=np.int64)
    for t in range(T):
        others = [u for u in range(T) if u != t]
        u = others[int(np.argmax(L[others]))]
        kh[t] = int(np.sum((Cc[:, u] - Cc[:, t]) >= (L[u] - L[t])))
    return bp, kh, sh, k1


def au_fit(r, count, B):
    """Shimodaira 2002: weighted least squares of z_k = -Phi^-1(count_k / B) on d sqrt(r_k) + c / sqrt(r_k)"""
    from scipy.stats import norm
    r = np.asarray(r, dtype=np.float64)
    cnt = np.asarray(count, dtype=np.int64)
    ok = (cnt > 0) & (cnt < B)
    if ok.sum() < 2:
        return {"au": cnt[k1_of(r)] / float(B), "d": 0.0, "c": 0.0, "rss": 0.0, "nused": int(ok.sum())}
    p = cnt[ok] / float(B)
    z = -norm.ppf(p)
    w = B * norm.pdf(z) ** 2 / (p * (1.0 - p))
    A = np.stack([np.sqrt(r[ok]), 1.0 / np.sqrt(r[ok])], axis=1)
    sw = np.sqrt(w)
    (d, c), *_ = np.linalg.lstsq(A * sw[:, None], z * sw, rcond=None)
    res = z - A @ np.array([d, c])
    return {"au": float(1.0 - norm.cdf(d - c)), "d": float(d), "c": float(c), "rss": float(np.sum(w * res * res)), "nused": int(ok.sum())}


def default_ndraws(N, scales=None):
    sc = np.arange(5, 15) / 10.0 if scales is None else np.asarray(scales, dtype=np.float64)
    return np.maximum(1, np.floor(sc * N + 0.5)).astype(np.int64)


def tests(site_lnl, B, seed, scales=None):
    """the whole table: counts, p-values and the AU fit of every tree"""
    X = np.asarray(site_lnl, dtype=np.float64)
    T, N = X.shape
    nd = default_ndraws(N, scales)
    bp, kh, sh, k1 = counts(X, nd, B, seed)
    r = nd / float(N)
    fits = [au_fit(r, bp[:, t], B) for t in range(T)]
    return {"bp_count": bp, "kh_count": kh, "sh_count": sh, "k1": k1, "ndraws": nd, "lnl": column_sums(X),
            "au": np.array([f["au"] for f in fits]), "fits": fits}


def synthetic_table(N=400, T=5, seed=7):
    """The fixture of the meaning tests: tree 0 the best, tree 1 a near tie, tree 2 worse, tree 3 a bit-identical copy of tree 0,
    tree 4 hopeless.  A gamma-distributed base column (per-site lnL are negative and skewed) plus normal perturbations."""
    rng = np.random.default_rng(seed)
    base = -rng.gamma(2.0, 1.5, size=N)
    X = np.empty((T, N))
    X[0] = base
    X[1] = base + rng.normal(-3.3 / N, 0.12, size=N)
    X[2] = base + rng.normal(-9.8 / N, 0.12, size=N)
    X[3] = X[0]
    X[4] = base + rng.normal(-187.0 / N, 0.25, size=N)
    for t in range(5, T):
        X[t] = base + rng.normal(-20.0 * t / N, 0.2, size=N)
    return X
