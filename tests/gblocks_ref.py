"""The block selection behind `-gblocks_trim`, restated in Python from the rule in include/peprml.h (Castresana 2000 and the
program's documentation; parity with the Gblocks binary is unpinned), independently of the library:

* procedure()    the published steps one after the other, as loops over blocks
* closed_form()  the same five steps as predicates on previous / next indices (numpy scans)
* defaults()     PEPR's parameters (MSATrimmer.java:94-98 and the program's documented defaults)

Bytes are compared by identity; '-' is the only gap byte."""
import math

import numpy as np

GAP = ord("-")
MISSING = ord("?")
NONE, HALF, ALL = 1, 2, 3
SEL1, SEL3, SEL4, KEPT = 16, 32, 64, 128


def defaults(n):
    b1 = math.ceil(n * 0.8)
    return {"b1": b1, "b2": max(b1, 85 * n // 100), "b3": 8, "b4": 10, "b0": 10, "gaps": HALF}


def resolve(n, params=None):
    p = dict(defaults(n))
    for k, v in (params or {}).items():
        if v:
            p[k] = v
    if not (n / 2 < p["b1"] <= p["b2"] <= n and p["b3"] >= 0 and p["b4"] >= 2 and p["b0"] >= 2 and p["gaps"] in (NONE, HALF, ALL)):
        raise ValueError("Gblocks parameters out of bounds: %r for %d rows" % (p, n))
    return p


def matrix(gene):
    rows = [r.encode("latin-1") if isinstance(r, str) else r for r in gene[1]]
    return np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(len(rows), -1) if rows and len(rows[0]) else np.zeros((len(rows), 0), np.uint8)


def classes(m, p):
    """-> (class per column, gap position per column)"""
    n, L = m.shape
    cls, gp = [], []
    for c in range(L):
        col = m[:, c].tolist()
        gaps = col.count(GAP)
        counts = {}
        for b in col:
            if b != GAP:
                counts[b] = counts.get(b, 0) + 1
        top = max(counts.values()) if counts else 0
        g = gaps > 0 if p["gaps"] == NONE else 2 * gaps >= n if p["gaps"] == HALF else False
        gp.append(g)
        cls.append(0 if g or top < p["b1"] else 2 if top >= p["b2"] else 1)
    return cls, gp


def _blocks(sel):
    """the maximal runs of selected columns as (first, last + 1)"""
    out, c, L = [], 0, len(sel)
    while c < L:
        if sel[c]:
            e = c
            while e < L and sel[e]:
                e += 1
            out.append((c, e))
            c = e
        else:
            c += 1
    return out


def procedure(cls, gp, p):
    """the five steps in order -> the selection after each step (the last: the kept columns), five lists of bool"""
    L = len(cls)
    sel = [True] * L
    for a, e in _blocks([x == 0 for x in cls]):                    # 1. long runs of non-conserved columns
        if e - a > p["b3"]:
            sel[a:e] = [False] * (e - a)
    s1 = list(sel)
    for a, e in _blocks(sel):                                      # 2. flanks: back to a highly conserved column on each side
        twos = [c for c in range(a, e) if cls[c] == 2]
        lo, hi = (twos[0], twos[-1] + 1) if twos else (e, e)
        sel[a:lo] = [False] * (lo - a)
        sel[hi:e] = [False] * (e - hi)
    s2 = list(sel)
    for a, e in _blocks(sel):                                      # 3. short initial blocks
        if e - a < p["b0"]:
            sel[a:e] = [False] * (e - a)
    s3 = list(sel)
    for g in [c for c in range(L) if s3[c] and gp[c]]:             # 4. gap positions and the non-conserved columns next to them
        sel[g] = False
        for step in (-1, 1):
            c = g + step
            while 0 <= c < L and s3[c] and cls[c] == 0:
                sel[c] = False
                c += step
    s4 = list(sel)
    for a, e in _blocks(sel):                                      # 5. short blocks
        if e - a < p["b4"]:
            sel[a:e] = [False] * (e - a)
    return s1, s2, s3, s4, sel


def _prev(mask):
    """index of the last True at or before each position, -1 when there is none"""
    idx = np.where(mask, np.arange(len(mask)), -1)
    return np.maximum.accumulate(idx) if len(mask) else idx


def _next(mask):
    L = len(mask)
    idx = np.where(mask, np.arange(L), L)
    return np.minimum.accumulate(idx[::-1])[::-1] if L else idx


def closed_form(cls, gp, p):
    cls, gp = np.asarray(cls, dtype=np.int64), np.asarray(gp, dtype=bool)
    nz = cls != 0
    s1 = ~(~nz & (_next(nz) - _prev(nz) - 1 > p["b3"]))
    two = cls == 2
    s2 = s1 & (_prev(two) > _prev(~s1)) & (_next(two) < _next(~s1))
    s3 = s2 & (_next(~s2) - _prev(~s2) - 1 >= p["b0"])
    z = s3 & ~nz
    hit = z & gp
    s4 = s3 & ~(z & ((_prev(hit) > _prev(~z)) | (_next(hit) < _next(~z))))
    kept = s4 & (_next(~s4) - _prev(~s4) - 1 >= p["b4"])
    return s1.tolist(), s2.tolist(), s3.tolist(), s4.tolist(), kept.tolist()


def flag_bytes(cls, gp, stages):
    """the byte per column that the library's test doors return"""
    s1, _, s3, s4, kept = stages
    return [c | (4 if g else 0) | (SEL1 if a else 0) | (SEL3 if b else 0) | (SEL4 if d else 0) | (KEPT if k else 0)
            for c, g, a, b, d, k in zip(cls, gp, s1, s3, s4, kept)]


def flags(gene, params=None):
    m = matrix(gene)
    p = resolve(m.shape[0], params)
    cls, gp = classes(m, p)
    return flag_bytes(cls, gp, procedure(cls, gp, p))


def trim(gene, params=None):
    """-> the dict Context.gblocks_trim returns for the gene"""
    m = matrix(gene)
    f = flags(gene, params)
    kept = [c for c, x in enumerate(f) if x & KEPT]
    rows = [m[r, kept].tobytes() for r in range(m.shape[0])]
    if gene[1] and isinstance(gene[1][0], str):
        rows = [r.decode("latin-1") for r in rows]
    return {"names": list(gene[0]), "rows": rows, "ncols": m.shape[1], "nkept": len(kept), "kept_cols": kept,
            "gap_or_missing": int(np.isin(m, (GAP, MISSING)).sum())}


RESIDUES = np.frombuffer(b"ARNDCQEGHILKMFPSTWYV", dtype=np.uint8)


def run_gene(rng, n, L):
    """uint8 [n, L] built from runs of 1-29 columns of four kinds: random residues, one residue with about 10 % of a second, one
    residue throughout, one residue with 5 / 30 / 60 % gaps"""
    m = np.empty((n, L), dtype=np.uint8)
    c = 0
    while c < L:
        w = min(int(rng.integers(1, 30)), L - c)
        kind = int(rng.integers(0, 4))
        a, b = RESIDUES[rng.choice(20, 2, replace=False)]
        if kind == 0:
            blk = RESIDUES[rng.integers(0, 20, (n, w))]
        elif kind == 1:
            blk = np.where(rng.random((n, w)) < 0.1, b, a).astype(np.uint8)
        elif kind == 2:
            blk = np.full((n, w), a, dtype=np.uint8)
        else:
            blk = np.where(rng.random((n, w)) < (0.05, 0.3, 0.6)[int(rng.integers(0, 3))], GAP, a).astype(np.uint8)
        m[:, c:c + w] = blk
        c += w
    return m


def gene_of(m, prefix="t"):
    return (["%s%03d" % (prefix, i) for i in range(m.shape[0])], [m[i].tobytes() for i in range(m.shape[0])])


def steps_exercised(stages):
    """which of the five steps deselected at least one column"""
    before = [[True] * len(stages[0])] + list(stages[:-1])
    return [any(a and not b for a, b in zip(x, y)) for x, y in zip(before, stages)]
