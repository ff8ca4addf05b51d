#!/usr/bin/env python
"""Times block trimming on the device ("Block-trimming kernels").

usage: measure_gblocks.py [--genes 500] [--taxa 200] [--cols 1000] [--seed 1] [--out FILE]
The genes are built from runs of 1-29 columns of four kinds (random residues, one residue with about 10 % of a second, one residue
throughout, one residue with 5 / 30 / 60 % gaps), so that every step of the selection has work.  A context with cfg.profile = 1;
one warm-up call of each kind on other data; then pml_gblocks_trim on the genes: pml_gblocks_stats' HIP-event times of k_gbclass,
k_gbselect and the host-to-device copy, pml_trim_stats' time of k_colgather, and the host clock around the whole call.  In the
same run pml_trim_columns (PML_TRIM_GAP_UNIFORM) on the same genes gives k_colclass on the same bytes.  Prints one JSON line."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pepr_amd import _lib, engine

RESIDUES = np.frombuffer(b"ARNDCQEGHILKMFPSTWYV", dtype=np.uint8)


def run_gene(rng, n, L):
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
            blk = np.where(rng.random((n, w)) < (0.05, 0.3, 0.6)[int(rng.integers(0, 3))], ord("-"), a).astype(np.uint8)
        m[:, c:c + w] = blk
        c += w
    return m


def alignments(mats, names, keep):
    """uint8 matrices [ntax, ncols] -> a pml_alignment array"""
    na = (C.c_char_p * len(names))(*[n.encode() for n in names])
    keep.append(na)
    out = (_lib.Alignment * len(mats))()
    for g, m in enumerate(mats):
        ra = (C.c_char_p * m.shape[0])(*[m[r].tobytes() for r in range(m.shape[0])])
        keep.append(ra)
        out[g] = _lib.Alignment(m.shape[0], m.shape[1], na, ra)
    return out


def main(argv):
    opt = {"genes": 500, "taxa": 200, "cols": 1000, "seed": 1, "out": ""}
    for i in range(0, len(argv) - 1, 2):
        key = argv[i].lstrip("-")
        opt[key] = type(opt[key])(argv[i + 1])
    G, n, m = opt["genes"], opt["taxa"], opt["cols"]
    rng = np.random.default_rng(opt["seed"])
    names = ["tx%04d" % i for i in range(n)]
    ctx = engine.Context(0, profile=True)
    L, keep = ctx.L, []

    def blocks(alns, count):
        res = _lib.TrimResult()
        t0 = time.perf_counter()
        ctx._check(L.pml_gblocks_trim(ctx.ptr, count, alns, None, C.byref(res)))
        return res, time.perf_counter() - t0

    def columns(alns, count):
        res = _lib.TrimResult()
        t0 = time.perf_counter()
        ctx._check(L.pml_trim_columns(ctx.ptr, count, alns, engine.TRIM_GAP_UNIFORM, C.byref(res)))
        return res, time.perf_counter() - t0

    warm = alignments([run_gene(rng, n, m) for _ in range(2)], names, keep)
    for call in (blocks, columns):
        res, _ = call(warm, 2)
        L.pml_trim_result_free(C.byref(res))
    alns = alignments([run_gene(rng, n, m) for _ in range(G)], names, keep)
    g0, t0 = ctx.gblocks_stats(), ctx.trim_stats()
    res, wall = blocks(alns, G)
    g1, t1 = ctx.gblocks_stats(), ctx.trim_stats()
    kept = sum(res.nkept[g] for g in range(G))
    L.pml_trim_result_free(C.byref(res))
    res, wall_columns = columns(alns, G)
    t2 = ctx.trim_stats()
    L.pml_trim_result_free(C.byref(res))
    cells = G * n * m
    gb = {k: g1[k] - g0[k] for k in g1}
    gather_ms = t1["gather_ms"] - t0["gather_ms"]
    colclass_ms = t2["class_ms"] - t1["class_ms"]
    line = {"genes": G, "taxa": n, "cols": m, "cells": cells, "kept_columns": kept, "k_gbclass_ms": gb["class_ms"], "k_gbselect_ms": gb["select_ms"],
            "k_colgather_ms": gather_ms, "h2d_copy_ms": gb["upload_ms"], "call_wall_ms": wall * 1e3, "class_launches": gb["class_launches"],
            "select_launches": gb["select_launches"], "k_gbclass_GBps_one_pass": cells / gb["class_ms"] / 1e6 if gb["class_ms"] else None,
            "k_colclass_ms_same_bytes": colclass_ms, "k_colclass_GBps": cells / colclass_ms / 1e6 if colclass_ms else None,
            "k_colclass_upload_ms": t2["upload_ms"] - t1["upload_ms"], "trim_columns_wall_ms": wall_columns * 1e3}
    print(json.dumps(line), flush=True)
    if opt["out"]:
        with open(opt["out"], "w") as f:
            f.write(json.dumps(line) + "\n")
    ctx.close()


if __name__ == "__main__":
    main(sys.argv[1:])
