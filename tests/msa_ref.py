"""The multiple-alignment rule of include/peprml.h ("Multiple alignment") in plain Python / numpy, written from the rule's text and
not from the C++: the guide tree, the profile-profile DP with its traceback, the merge and the progressive alignment of a set.
Integers are Python's or int64: nothing here can overflow where int32 would.  Alignments are lists of texts, `-` a gap."""
import numpy as np

import sw_ref
from sw_ref import PLAIN, asym_tables, mutate, random_protein  # noqa: F401 -- the generators the tests share

NEG = -(10 ** 15)
LETTERS = sw_ref.ORDER


def encode_row(text):
    """codes of an aligned row, 23 in a gap cell"""
    return np.asarray([23 if ch == "-" else int(sw_ref.encode(ch)[0]) for ch in text], dtype=np.int64)


def counts(rows):
    """[L][23]: the rows with code a in column i"""
    L = len(rows[0])
    assert all(len(r) == L for r in rows)
    c = np.zeros((L, 23), dtype=np.int64)
    for r in rows:
        codes = encode_row(r)
        for i in np.nonzero(codes < 23)[0]:
            c[i, codes[i]] += 1
    return c


def column_scores(X, Y, table):
    """s[i][j] = sum_a sum_b cX[i][a] cY[j][b] T[a][b], (LX, LY)"""
    T = np.asarray(table, dtype=np.int64).reshape(24, 24)[:23, :23]
    return counts(X) @ T @ counts(Y).T


def bound(nX, nY, LX, LY, table, gap_open=11, gap_extend=1):
    """the left side of the rule's int32 bound: refused when >= 2^30"""
    M = int(np.abs(np.asarray(table, dtype=np.int64).reshape(24, 24)[:23, :23]).max())
    return nX * nY * ((M + gap_open) * (min(LX, LY) + 1) + gap_extend * (LX + LY))


def matrices(X, Y, table, gap_open=11, gap_extend=1):
    """H, E, F as (LX + 1) x (LY + 1) int64 arrays, NEG where a term does not exist.  Row by row: F and the diagonal are
    vectors over the columns, E is a running scan"""
    LX, LY = len(X[0]), len(Y[0])
    w = len(X) * len(Y)
    GO, GE = gap_open * w, gap_extend * w
    s = column_scores(X, Y, table)
    H = np.full((LX + 1, LY + 1), NEG, dtype=np.int64)
    E = np.full((LX + 1, LY + 1), NEG, dtype=np.int64)
    F = np.full((LX + 1, LY + 1), NEG, dtype=np.int64)
    oF = np.full(LY + 1, GO, dtype=np.int64)
    oF[0] = oF[LY] = 0
    for i in range(LX + 1):
        oE = 0 if i in (0, LX) else GO
        D = np.full(LY + 1, NEG, dtype=np.int64)                     # everything but E
        if i >= 1:
            F[i] = np.maximum(F[i - 1] - GE, H[i - 1] - oF - GE)
            D = F[i].copy()
            D[1:] = np.maximum(D[1:], H[i - 1][:-1] + s[i - 1])
        if i == 0:
            D[0] = 0
        Dl = D.tolist()
        h, e = Dl[0], NEG
        hs, es = [h], [NEG]
        for j in range(1, LY + 1):
            e = max(e - GE, h - oE - GE)
            h = max(Dl[j], e)
            hs.append(h)
            es.append(e)
        H[i], E[i] = hs, es
    return H, E, F, s, GO, GE


def profile_align(X, Y, table=None, gap_open=11, gap_extend=1):
    """-> (score, path, rows): path per merged column 0 = both, 1 = Y's column only (E), 2 = X's only (F); rows = X's, then Y's"""
    table = sw_ref.blosum62() if table is None else table
    LX, LY = len(X[0]), len(Y[0])
    H, E, F, s, GO, GE = matrices(X, Y, table, gap_open, gap_extend)
    H, E, F = H.tolist(), E.tolist(), F.tolist()
    i, j, state, path = LX, LY, "H", []
    while i > 0 or j > 0:
        if state == "H":
            if i > 0 and j > 0 and H[i][j] == H[i - 1][j - 1] + int(s[i - 1, j - 1]):
                path.append(0)
                i, j = i - 1, j - 1
            elif j > 0 and H[i][j] == E[i][j]:
                state = "E"
            else:
                assert i > 0 and H[i][j] == F[i][j]
                state = "F"
        elif state == "E":
            path.append(1)
            if E[i][j] == H[i][j - 1] - (0 if i in (0, LX) else GO) - GE:
                state = "H"
            j -= 1
        else:
            path.append(2)
            if F[i][j] == H[i - 1][j] - (0 if j in (0, LY) else GO) - GE:
                state = "H"
            i -= 1
    path.reverse()
    return int(H[LX][LY]), path, merge_rows(X, Y, path)


def merge_rows(X, Y, path):
    out = [[] for _ in range(len(X) + len(Y))]
    i = j = 0
    for p in path:
        for r, row in enumerate(X):
            out[r].append(row[i] if p != 1 else "-")
        for r, row in enumerate(Y):
            out[len(X) + r].append(row[j] if p != 2 else "-")
        i += p != 1
        j += p != 2
    return ["".join(r) for r in out]


def guide_tree(S):
    """S[a][b], a < b -> [(x, y, level)]: the largest average over the cross pairs, compared by cross multiplication in
    Python integers, ties to the lowest first id, then the lowest second id"""
    n = len(S)
    members = {k: [k] for k in range(n)}
    level = {k: 0 for k in range(n)}
    merges = []
    while len(members) > 1:
        best = None
        ids = sorted(members)
        for ai, a in enumerate(ids):
            for b in ids[ai + 1:]:
                tot = sum(int(S[min(p, q)][max(p, q)]) for p in members[a] for q in members[b])
                cnt = len(members[a]) * len(members[b])
                if best is None or tot * best[1] > best[0] * cnt:
                    best = (tot, cnt, a, b)
        _, _, a, b = best
        level[a] = 1 + max(level[a], level[b])
        members[a] = members[a] + members.pop(b)
        merges.append((a, b, level[a]))
    return merges


def clean(text):
    """a residue text as the rule encodes and prints it: upper case, J O U as X"""
    return "".join(LETTERS[c] for c in sw_ref.encode(text))


def pair_scores(seqs, table=None, gap_open=11, gap_extend=1):
    n = len(seqs)
    S = [[0] * n for _ in range(n)]
    for a in range(n):
        for b in range(a + 1, n):
            S[a][b] = sw_ref.score(seqs[a], seqs[b], table, gap_open, gap_extend)
    return S


def align_set(seqs, table=None, gap_open=11, gap_extend=1):
    """-> {"rows": aligned texts in input order, "merges": [(x, y, level, score)]}"""
    table = sw_ref.blosum62() if table is None else table
    for k, s in enumerate(seqs):
        if not s:
            raise ValueError("sequence %d is empty" % k)
    merges = guide_tree(pair_scores(seqs, table, gap_open, gap_extend))
    rows = {k: [clean(s)] for k, s in enumerate(seqs)}
    order = {k: [k] for k in range(len(seqs))}
    out = []
    for x, y, lv in merges:
        assert bound(len(rows[x]), len(rows[y]), len(rows[x][0]), len(rows[y][0]), table, gap_open, gap_extend) < 2 ** 30
        score, _, merged = profile_align(rows[x], rows[y], table, gap_open, gap_extend)
        rows[x] = merged
        order[x] = order[x] + order.pop(y)
        del rows[y]
        out.append((x, y, lv, score))
    final = [None] * len(seqs)
    for r, k in enumerate(order[0]):
        final[k] = rows[0][r]
    return {"rows": final, "merges": out}


# ---- inputs the tests share ----
def family(rng, n, length, frac=0.08, deletions=0, del_len=4, truncate=False, alphabet=PLAIN):
    """n mutants of one ancestor of `length` residues: substitutions at rate frac; `deletions` runs of del_len residues cut out of
    every second member; with truncate the head of member 1 cut and a tail appended to member 2"""
    root = random_protein(rng, length, alphabet)
    out = []
    for k in range(n):
        s = mutate(rng, root, frac)
        if deletions and k % 2 == 1:
            for _ in range(deletions):
                at = int(rng.integers(del_len, max(len(s) - 2 * del_len, del_len + 1)))
                s = s[:at] + s[at + del_len:]
        if truncate and k == 1:
            s = s[min(5, len(s) - 1):]
        if truncate and k == 2:
            s = s + random_protein(rng, 6, PLAIN)
        out.append(s)
    return out


def random_profile(rng, n, L, gap_frac=0.2):
    """n rows of L columns, gaps at rate gap_frac, no row empty"""
    rows = []
    for _ in range(n):
        r = list(random_protein(rng, L, PLAIN))
        for k in range(L):
            if rng.random() < gap_frac:
                r[k] = "-"
        if all(ch == "-" for ch in r):
            r[int(rng.integers(0, L))] = "A"
        rows.append("".join(r))
    return rows


def degap(row):
    return row.replace("-", "")
