"""The weighted tree selection tests (wKH, wSH) restated in numpy from their definitions (include/peprml.h, "weighted"): the
reference of tests/test_tree_tests_weighted_host.py and tests/test_gpu_tree_tests_weighted.py.  Draws, replicate sums and
column sums are those of tests/rell_ref.py; nothing here is shared with the library.

  sigma_ut   d_s = X[u][s] - X[t][s], mean = (sum_s d_s) / N, sigma_ut^2 = N / (N - 1) sum_s (d_s - mean)^2: np.longdouble, two
             passes, rounded to double at the end; inv_sigma = 1 / sigma in double, 0 where sigma = 0 and on the diagonal
  ratios     (a - b) * inv_sigma: the rounded difference, then one rounded multiply (as rell_ref.counts forms C_t)
  counts     wsh[t] = #{max_u (C_u - C_t) is_ut >= S_t}, S_t = max_u (L_u - L_t) is_ut; wkh[t] = #{(C_u* - C_t) is_u*t >= S_t},
             u* = the argmax of S_t (first of equals); u != t with is_ut > 0; a tree with no such u counts every replicate
  margins    how far every comparison above is from flipping, relative: the GPU tests assert exact equality of integer
             counts, which only holds if no comparison is within the rounding of sigma (a few 1e-16) of a tie
"""
import functools

import numpy as np

import rell_ref

TINY = np.finfo(np.float64).tiny


def pair_sigma(site_lnl):
    """sigma[T, T] in double from longdouble two-pass sums (0 on the diagonal; 0 for N = 1 and identical columns)"""
    X = np.asarray(site_lnl, dtype=np.float64).astype(np.longdouble)
    T, N = X.shape
    sig = np.zeros((T, T))
    if N < 2:
        return sig
    for u in range(T):
        for t in range(u + 1, T):
            d = X[u] - X[t]
            mean = d.sum() / np.longdouble(N)
            e = d - mean
            var = (e * e).sum() * (np.longdouble(N) / np.longdouble(N - 1))
            sig[u, t] = sig[t, u] = float(np.sqrt(var))
    return sig


def inv_of(sigma):
    out = np.zeros_like(sigma)
    nz = sigma > 0
    out[nz] = 1.0 / sigma[nz]
    return out


def weighted_ref(site_lnl, ndraws, B, seed, Y=None, inv_sigma=None):
    """-> dict: sigma, inv_sigma [T, T]; S [T] (-inf: no pair), ustar [T] (-1: no pair); wkh, wsh [T] integer counts; k1;
    margin_wsh, margin_wkh, margin_ustar: the smallest relative distance of any comparison from a tie (inf if there is none).
    Two candidates u whose observed ratios are EQUAL (bit-identical columns) are not a near-tie: equal inputs give equal
    ratios in any implementation that treats every pair alike, and the rule (first of equals) decides."""
    X = np.asarray(site_lnl, dtype=np.float64)
    T, N = X.shape
    nd = np.asarray(ndraws, dtype=np.int64)
    if Y is None:
        Y = rell_ref.replicate_sums(X, nd, B, seed)
    L = rell_ref.column_sums(X)
    k1 = rell_ref.k1_of(nd / float(N))
    Cc = Y[k1] * (float(N) / float(nd[k1])) - L[None, :]
    sigma = pair_sigma(X)
    isg = inv_of(sigma) if inv_sigma is None else np.asarray(inv_sigma, dtype=np.float64)
    S = np.full(T, -np.inf)
    ustar = np.full(T, -1, dtype=np.int64)
    wkh = np.zeros(T, dtype=np.int64)
    wsh = np.zeros(T, dtype=np.int64)
    m_wsh = m_wkh = m_us = np.inf

    def rel(a, b):
        return np.abs(a - b) / np.maximum(np.maximum(np.abs(a), np.abs(b)), TINY)
    for t in range(T):
        us = [u for u in range(T) if u != t and isg[t, u] > 0]
        if not us:
            wkh[t] = wsh[t] = Y.shape[1]
            continue
        w = isg[t, us]
        q_obs = (L[us] - L[t]) * w
        j = int(np.argmax(q_obs))                                              # the first of equals
        S[t], ustar[t] = q_obs[j], us[j]
        others = q_obs[q_obs != q_obs[j]]
        if len(others):
            m_us = min(m_us, float(rel(others.max(), q_obs[j])))
        q = (Cc[:, us] - Cc[:, [t]]) * w[None, :]                              # [B, pairs]
        s_star = q.max(axis=1)
        wsh[t] = int(np.sum(s_star >= S[t]))
        wkh[t] = int(np.sum(q[:, j] >= S[t]))
        m_wsh = min(m_wsh, float(rel(s_star, S[t]).min()))
        m_wkh = min(m_wkh, float(rel(q[:, j], S[t]).min()))
    return {"sigma": sigma, "inv_sigma": isg, "S": S, "ustar": ustar, "wkh": wkh, "wsh": wsh, "k1": k1, "L": L,
            "margin_wsh": m_wsh, "margin_wkh": m_wkh, "margin_ustar": m_us}


# ---- the cases the GPU tests run; the host test checks the margins of every one of them -------------------------------------

def table(N, T, seed):
    """per-site lnL of T trees that share a gamma-distributed base column, with perturbations whose spread GROWS with the tree
    index (unequal pairwise variances); T >= 4: tree 3 is a bit-identical copy of tree 0 (an excluded pair)"""
    rng = np.random.default_rng(seed)
    base = -rng.gamma(2.0, 1.5, size=N)
    spread = 0.05 + 0.25 * np.arange(T) / max(T - 1, 1)
    X = base[None, :] + rng.normal(0.0, 1.0, size=(T, N)) * spread[:, None] - 0.002 * np.arange(T)[:, None]
    if T >= 4:
        X[3] = X[0]
    return X


def ndraws_of(N, K):
    return np.array([N], dtype=np.int64) if K == 1 else rell_ref.default_ndraws(N)


SIGMA_CASES = [(200, 2), (200, 3), (200, 5), (200, 64), (1, 5), (7, 5), (4099, 5), (4099, 64)]       # (N, T) of the k_rell_pairsd grid
COUNT_N = 200
COUNT_CASES = [(K, B, T) for K in (1, 10) for B in (37, 1000) for T in (2, 3, 5, 64)]                # at N = COUNT_N
DEGENERATE_CASES = [(1, 5), (7, 5)]                                                                  # (N, T), K = 1, B = 37


def case_seed(N, T, K, B):
    return 1000 * N + 17 * T + 3 * K + B


@functools.lru_cache(maxsize=None)
def case(N, T, K, B):
    """(X, ndraws, seed, Y, reference) of one case, computed once and shared; treat as read-only"""
    seed = case_seed(N, T, K, B)
    X = table(N, T, seed)
    nd = ndraws_of(N, K)
    Y = rell_ref.replicate_sums(X, nd, B, seed)
    for a in (X, nd, Y):
        a.setflags(write=False)
    return X, nd, seed, Y, weighted_ref(X, nd, B, seed, Y=Y)


def all_count_cases():
    return [(COUNT_N, T, K, B) for K, B, T in COUNT_CASES] + [(N, T, 1, 37) for N, T in DEGENERATE_CASES]


def unequal_variance_table(N=400, seed=3):
    """three trees: the best, a near neighbour whose per-site lnL differs from the best's by little at every site (one NNI: small
    sigma), and a far tree whose per-site differences are large (several moves: large sigma) though its total is not much worse.
    Plain SH measures the neighbour against max_u C_u, which the far tree's spread dominates; the weighted form does not."""
    rng = np.random.default_rng(seed)
    base = -rng.gamma(2.0, 1.5, size=N)
    X = np.empty((3, N))
    X[0] = base
    X[1] = base + rng.normal(-2.0 / N, 0.03, size=N)
    X[2] = base + rng.normal(-45.0 / N, 0.9, size=N)
    return X
