"""The homology-search rule of include/peprml.h ("Homology search") in plain Python / numpy, written from the rule's text and not from
the C++: encoding, the O(mn) affine-gap Smith-Waterman score, the per-genome selection, statistics, the table and the
traceback.  genomes: a list of genomes, each a list of (title, residues)."""
import math

import numpy as np

ORDER = "ARNDCQEGHILKMFPSTWYVBZX"
NEG = -(10 ** 9)


def blosum62():
    """24 x 24, the table as loaded (engine.blosum62_as_loaded)"""
    from pepr_amd import engine
    return np.asarray(engine.blosum62_as_loaded(), dtype=np.int64).reshape(24, 24)


def encode(text):
    out = []
    for k, ch in enumerate(text.upper()):
        if ch in "JOU":
            ch = "X"
        if ch not in ORDER:
            raise ValueError("byte %r at position %d" % (ch, k))
        out.append(ORDER.index(ch))
    return np.asarray(out, dtype=np.int64)


def matrices(q, t, table, gap_open=11, gap_extend=1):
    """H, E, F as (m + 1) x (n + 1) arrays of Python-exact integers; row and column 0 are the boundary"""
    m, n = len(q), len(t)
    H = np.zeros((m + 1, n + 1), dtype=np.int64)
    E = np.full((m + 1, n + 1), NEG, dtype=np.int64)
    F = np.full((m + 1, n + 1), NEG, dtype=np.int64)
    oe = gap_open + gap_extend
    for i in range(1, m + 1):
        sub = table[q[i - 1]][t] if n else None
        for j in range(1, n + 1):
            E[i, j] = max(E[i, j - 1] - gap_extend, H[i, j - 1] - oe)
            F[i, j] = max(F[i - 1, j] - gap_extend, H[i - 1, j] - oe)
            H[i, j] = max(0, H[i - 1, j - 1] + sub[j - 1], E[i, j], F[i, j])
    return H, E, F


def score(qtext, ttext, table=None, gap_open=11, gap_extend=1):
    """S of one pair.  Row by row with numpy over the columns: F and the diagonal are vectors, E is a running scan."""
    table = blosum62() if table is None else table
    q, t = encode(qtext), encode(ttext)
    m, n = len(q), len(t)
    if not m or not n:
        return 0
    oe = gap_open + gap_extend
    Hp = np.zeros(n + 1, dtype=np.int64)
    Fp = np.full(n + 1, NEG, dtype=np.int64)
    best = 0
    for i in range(m):
        F = np.maximum(Fp - gap_extend, Hp - oe)
        D = np.zeros(n + 1, dtype=np.int64)
        D[1:] = np.maximum(np.maximum(Hp[:-1] + table[q[i]][t], F[1:]), 0)       # everything but E
        # H[j] = max(D[j], E[j]), E[j] = max(E[j-1] - ext, H[j-1] - oe): a sequential scan
        H = np.zeros(n + 1, dtype=np.int64)
        e = NEG
        h = 0
        Dl = D.tolist()
        out = [0] * (n + 1)
        for j in range(1, n + 1):
            e = max(e - gap_extend, h - oe)
            h = max(Dl[j], e)
            out[j] = h
        H[:] = out
        best = max(best, int(H.max()))
        Hp, Fp = H, F
    return best


def traceback(qtext, ttext, table=None, gap_open=11, gap_extend=1):
    """(pident text, length, mismatch, gapopen, qstart, qend, sstart, send) of the rule's one optimal alignment"""
    table = blosum62() if table is None else table
    q, t = encode(qtext), encode(ttext)
    H, E, F = matrices(q, t, table, gap_open, gap_extend)
    best = int(H.max())
    if best <= 0:
        return ("0.00", 0, 0, 0, 0, 0, 0, 0)
    bi, bj = [int(x) for x in np.argwhere(H == best)[0]]            # argwhere is row-major: the first maximal cell
    oe = gap_open + gap_extend
    i, j, state = bi, bj, "H"
    length = ident = mismatch = gapopen = 0
    while True:
        if state == "H":
            if H[i, j] == 0:
                break
            if H[i, j] == H[i - 1, j - 1] + table[q[i - 1]][t[j - 1]]:
                length += 1
                if q[i - 1] == t[j - 1]:
                    ident += 1
                else:
                    mismatch += 1
                i, j = i - 1, j - 1
            elif H[i, j] == E[i, j]:
                state, gapopen = "E", gapopen + 1
            else:
                state, gapopen = "F", gapopen + 1
        elif state == "E":
            length += 1
            if E[i, j] == H[i, j - 1] - oe:
                state = "H"
            j -= 1
        else:
            length += 1
            if F[i, j] == H[i - 1, j] - oe:
                state = "H"
            i -= 1
    return ("%.2f" % (100.0 * ident / length), length, mismatch, gapopen, i + 1, bi, j + 1, bj)


def label_of(title):
    parts = title.split()
    return parts[0] if parts else ""


def search(genomes, gap_open=11, gap_extend=1, lambda_=0.267, K=0.041, evalue=0.1, traceback_=False, table=None):
    """-> {"table": bytes, "hits": [(query index, subject index, target genome, S, bits, E)], "cells", "margin": the smallest
    relative distance of a winner's E from the cutoff}"""
    table = blosum62() if table is None else table
    flat = [(g, k, label_of(title), res) for g, genome in enumerate(genomes) for k, (title, res) in enumerate(genome)]
    for _, _, _, res in flat:
        encode(res)
        if len(res) > 65535:
            raise ValueError("too long")
    first = [0]
    for genome in genomes:
        first.append(first[-1] + len(genome))
    nres = [sum(len(res) for _, res in genome) for genome in genomes]
    cache = {}
    lines, hits, margin = [], [], float("inf")
    for g in range(len(genomes)):
        for qi, (_, _, qlabel, qres) in enumerate(flat):
            if not qres:
                continue
            win, wins = None, -1
            for k, (_, sres) in enumerate(genomes[g]):
                if not sres:
                    continue
                key = (qres.upper(), sres.upper())
                if key not in cache:
                    cache[key] = score(qres, sres, table, gap_open, gap_extend)
                if cache[key] > wins:                                 # strict: ties to the lowest position
                    win, wins = k, cache[key]
            if win is None or wins <= 0:
                continue
            e = K * len(qres) * nres[g] * math.exp(-lambda_ * wins)
            margin = min(margin, abs(e - evalue) / evalue)
            if not e <= evalue:
                continue
            bits = (lambda_ * wins - math.log(K)) / math.log(2.0)
            si = first[g] + win
            mid = "\t".join(str(x) for x in traceback(qres, flat[si][3], table, gap_open, gap_extend)) if traceback_ else "\t".join("0" * 8)
            lines.append("%s\t%s\t%s\t%.2e\t%.1f\n" % (qlabel, flat[si][2], mid, e, bits))
            hits.append((qi, si, g, wins, bits, e))
    cells = sum(len(r[3]) for r in flat) * sum(nres)
    return {"table": "".join(lines).encode(), "hits": hits, "cells": cells, "margin": margin}


# ---- inputs the tests share ----
ALPHABET = "ARNDCQEGHILKMFPSTWYVBZXJOUarndcqeghilkmfpstwyvbzxjou"
PLAIN = "ARNDCQEGHILKMFPSTWYV"


def random_protein(rng, n, alphabet=ALPHABET):
    return "".join(alphabet[i] for i in rng.integers(0, len(alphabet), n))


def mutate(rng, text, frac=0.05):
    out = list(text)
    for k in range(len(out)):
        if rng.random() < frac:
            out[k] = PLAIN[rng.integers(0, 20)]
    return "".join(out)


NO_P = PLAIN.replace("P", "")         # partners of a P flank: no P, no B Z X J O U, no lower case


def gap_subjects(p, at, flank=12):
    """pieces of p around row `at` with three residues cut out (the query's rows at - 1 .. at + 1 face a gap: F crosses the
    boundary) and with three put in (E)"""
    lo, hi = max(at - flank, 0), min(at + flank, len(p))
    cut = p[lo:max(at - 1, lo)] + p[min(at + 2, hi):hi]
    put = p[lo:at] + "WCW" + p[at:hi]
    return [cut, put]


def asym_tables(seed=62):
    """two 24 x 24 tables that are not their own transpose: (mild) BLOSUM62 with 3 subtracted above the diagonal, (wild) seeded
    uniform integers over all of int8 with both ends of the range planted, 127 on the diagonal too"""
    mild = blosum62().copy()
    mild[np.triu_indices(24, 1)] -= 3
    wild = np.random.default_rng(seed).integers(-128, 128, (24, 24)).astype(np.int64)
    wild[0][1], wild[1][0], wild[17][17] = 127, -128, 127
    return mild, wild


def flanked(core, total, at):
    """core inside a run of P, `total` residues in all.  Against a partner out of NO_P every BLOSUM62 score of a P row is
    negative: the rows before the core leave H = 0 and F below zero, the rows behind it never raise the maximum, so
    score(flanked(core, total, at), s) == score(core, s), and the same with the flank on the subject's side"""
    assert 0 <= at and at + len(core) <= total
    return "P" * at + core + "P" * (total - at - len(core))


def stream_chunks(lengths, chunk_bytes):
    """the rule of DESIGN.md "Homology search" by which one genome's subjects are laid out: ordered by length (stably), a boundary
    code behind each, a chunk closed before the subject that would take it past chunk_bytes (one longer subject is a chunk alone)
    -> (stream bytes of every chunk, the chunk of every subject by file position)"""
    order = sorted((k for k in range(len(lengths)) if lengths[k] > 0), key=lambda k: lengths[k])
    sizes, where = [], {}
    for k in order:
        if not sizes or sizes[-1] + lengths[k] + 1 > chunk_bytes:
            sizes.append(0)
        sizes[-1] += lengths[k] + 1
        where[k] = len(sizes) - 1
    return sizes, where


def planted_families(seed=5, ngenomes=3, nfam=3, length=60):
    rng = np.random.default_rng(seed)
    roots = [random_protein(rng, length, PLAIN) for _ in range(nfam)]
    return [[("g%d_f%d [genome %d]" % (g, f, g), mutate(rng, roots[f])) for f in range(nfam)] for g in range(ngenomes)]
