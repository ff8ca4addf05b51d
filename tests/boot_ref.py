"""The column bootstrap's rules (include/peprml.h pml_bootstrap2, csrc/boot.hpp) restated in Python / numpy: mix64, the key and
the draw; the counts from a per-gene first-occurrence pattern numbering of the text; the compaction; and materialise(), the
resampled text of a replicate.  Nothing here touches the library's encoder or its kernels (materialise uses engine.concatenate,
host text only)."""
import numpy as np

M64 = (1 << 64) - 1


def mix64(z):
    z &= M64
    z ^= z >> 30; z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 27; z = (z * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def key_of(seed, rep):
    return mix64(((seed + 1) * 0x9E3779B97F4A7C15 + rep) & M64)


def draw(key, j, ncols):
    return ((mix64(key + j) >> 32) * ncols) >> 32


def _mix64_np(z):
    z = z.copy()
    z ^= z >> np.uint64(30); z *= np.uint64(0xBF58476D1CE4E5B9)
    z ^= z >> np.uint64(27); z *= np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def draws(seed, rep, ncols, js=None):
    """columns c_j of replicate `rep` for j in js (default: all of 0..ncols-1), vectorised; equals draw() entry by entry"""
    js = np.arange(ncols, dtype=np.uint64) if js is None else np.asarray(js, dtype=np.uint64)
    with np.errstate(over="ignore"):
        h = _mix64_np(np.uint64(key_of(seed, rep)) + js) >> np.uint64(32)
        return ((h * np.uint64(ncols)) >> np.uint64(32)).astype(np.int64)


AA = "ARNDCQEGHILKMFPSTWYV"


def code_of(ch):
    """the residue code table of peprml.h: 0..19 the amino acids (either case), 20 = B, 21 = Z, 22 = anything else"""
    u = ch.upper()
    return AA.index(u) if u in AA else 20 if u == "B" else 21 if u == "Z" else 22


def col2pat(genes, sel=None):
    """pattern id of every column of the selection, genes in selection order: per gene the distinct columns of its text (two
    columns are the same pattern when their residue codes agree: X, - and ? are one code) are numbered by first occurrence, ids
    continue from gene to gene -> (int array[L], P)"""
    sel = list(range(len(genes))) if sel is None else list(sel)
    out, off = [], 0
    for g in sel:
        rows = genes[g][1]
        seen = {}
        for s in range(len(rows[0])):
            out.append(off + seen.setdefault(tuple(code_of(r[s]) for r in rows), len(seen)))
        off += len(seen)
    return np.array(out, dtype=np.int64), off


def counts(genes, sel, seed, rep):
    c2p, P = col2pat(genes, sel)
    return np.bincount(c2p[draws(seed, rep, len(c2p))], minlength=P)


def compact(count):
    return np.flatnonzero(count > 0)


def materialise(genes, sel, seed, rep):
    """the resampled text of replicate `rep`: the concatenation's columns c_0 .. c_{L-1} -> (names, rows)"""
    from pepr_amd import engine
    names, rows = engine.concatenate(genes, sel)
    m = np.array([list(r) for r in rows])
    cols = draws(seed, rep, m.shape[1])
    return names, ["".join(r) for r in m[:, cols]]
