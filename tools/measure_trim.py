#!/usr/bin/env python
"""Times column trimming on the device ("Column trimming").

usage: measure_trim.py [--genes 500] [--taxa 200] [--cols 1000] [--runs 3] [--seed 1] [--out FILE]
Part 1  random bytes (1..255), PML_TRIM_UNIFORM, a context with cfg.profile = 1: pml_trim_stats' HIP-event times of k_colclass and
        k_colgather next to the HIP-event time of the host-to-device copy of the same bytes in the same call, after one warm-up
        call on other data.
Part 2  the chained call (pml_trim_congruence_filter) against pml_trim_columns followed by pml_congruence_filter on the returned
        rows, the same process, alternating, wall time around the C calls (each ends in a stream synchronise).  The genes are
        evolved down one random tree (8 % change per branch, 3 % gaps) and end in a block of one-residue columns: columns of
        uniformly random bytes give every split a count of 1, which makes the congruence stage's kept set every split of the
        call -- a case no alignment produces and its cost kernel is not meant for.
Prints one JSON line per part."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pepr_amd import _lib, engine


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


def evolved(rng, ngenes, ntax, ncols, block):
    letters = np.frombuffer(b"ARNDCQEGHILKMFPSTWYV", dtype=np.uint8)
    width = ngenes * ncols
    seq = {2 * ntax - 2: rng.integers(0, 20, width, dtype=np.uint8)}
    nodes, nxt, children = list(range(ntax)), ntax, {}
    while len(nodes) > 1:
        i, j = sorted(rng.choice(len(nodes), 2, replace=False))
        children[nxt] = (nodes[i], nodes[j])
        nodes = [x for k, x in enumerate(nodes) if k not in (i, j)] + [nxt]
        nxt += 1
    stack = [2 * ntax - 2]
    while stack:
        v = stack.pop()
        for c in children.get(v, ()):
            s = seq[v].copy()
            hit = rng.random(width) < 0.08
            s[hit] = rng.integers(0, 20, int(hit.sum()), dtype=np.uint8)
            seq[c] = s
            stack.append(c)
        if v >= ntax:
            del seq[v]
    full = np.stack([letters[seq[t]] for t in range(ntax)])
    full[rng.random(full.shape) < 0.03] = ord("-")
    tail = np.full((ntax, block), ord("A"), dtype=np.uint8)
    return [np.concatenate([full[:, g * ncols:(g + 1) * ncols], tail], axis=1) for g in range(ngenes)]


def main(argv):
    opt = {"genes": 500, "taxa": 200, "cols": 1000, "runs": 3, "seed": 1, "out": ""}
    for i in range(0, len(argv) - 1, 2):
        key = argv[i].lstrip("-")
        opt[key] = type(opt[key])(argv[i + 1])
    G, n, m = opt["genes"], opt["taxa"], opt["cols"]
    rng = np.random.default_rng(opt["seed"])
    names = ["tx%04d" % i for i in range(n)]
    ctx = engine.Context(0, profile=True)
    L, keep, lines = ctx.L, [], []

    def trim(alns, count):
        res = _lib.TrimResult()
        ctx._check(L.pml_trim_columns(ctx.ptr, count, alns, engine.TRIM_UNIFORM, C.byref(res)))
        return res

    # ---- part 1 ----
    warm = alignments([rng.integers(1, 256, (n, m), dtype=np.uint8) for _ in range(2)], names, keep)
    L.pml_trim_result_free(C.byref(trim(warm, 2)))
    alns = alignments([rng.integers(1, 256, (n, m), dtype=np.uint8) for _ in range(G)], names, keep)
    before = ctx.trim_stats()
    t0 = time.perf_counter()
    res = trim(alns, G)
    wall = time.perf_counter() - t0
    after = ctx.trim_stats()
    kept = sum(res.nkept[g] for g in range(G))
    L.pml_trim_result_free(C.byref(res))
    cells = G * n * m
    d = {k: after[k] - before[k] for k in after}
    lines.append({"part": "kernels", "genes": G, "taxa": n, "cols": m, "cells": cells, "kept_columns": kept, "k_colclass_ms": d["class_ms"],
                  "k_colgather_ms": d["gather_ms"], "h2d_copy_ms": d["upload_ms"], "class_launches": d["class_launches"],
                  "gather_launches": d["gather_launches"], "k_colclass_GBps": cells / d["class_ms"] / 1e6 if d["class_ms"] else None,
                  "k_colgather_GBps_read_plus_written": 2 * n * kept / d["gather_ms"] / 1e6 if d["gather_ms"] else None,
                  "h2d_GBps": cells / d["upload_ms"] / 1e6 if d["upload_ms"] else None, "call_wall_ms": wall * 1e3})
    print(json.dumps(lines[-1]), flush=True)
    del alns, warm
    keep.clear()

    # ---- part 2 ----
    alns = alignments(evolved(rng, G, n, m, m // 4), names, keep)
    flags = (C.c_int * G)()

    def chained():
        t0 = time.perf_counter()
        tres, cres = _lib.TrimResult(), _lib.CongruenceResult()
        ctx._check(L.pml_trim_congruence_filter(ctx.ptr, G, alns, engine.TRIM_UNIFORM, 0.1, flags, C.byref(tres), C.byref(cres)))
        dt = time.perf_counter() - t0
        out = (list(flags), list(cres.mean_cost[:G]), sum(tres.nkept[g] for g in range(G)))
        L.pml_trim_result_free(C.byref(tres)); L.pml_congruence_result_free(C.byref(cres))
        return dt, out

    def two_calls():
        t0 = time.perf_counter()
        tres = trim(alns, G)
        second = (_lib.Alignment * G)()
        for g in range(G):                         # the returned rows go in as they are: no copy on the Python side
            second[g] = _lib.Alignment(tres.ntax[g], tres.nkept[g], alns[g].names, C.cast(tres.rows[g], C.POINTER(C.c_char_p)))
        cres = _lib.CongruenceResult()
        ctx._check(L.pml_congruence_filter(ctx.ptr, G, second, 0.1, flags, C.byref(cres)))
        dt = time.perf_counter() - t0
        out = (list(flags), list(cres.mean_cost[:G]), sum(tres.nkept[g] for g in range(G)))
        L.pml_trim_result_free(C.byref(tres)); L.pml_congruence_result_free(C.byref(cres))
        return dt, out

    chained(); two_calls()                          # warm-up: code objects, the first allocations
    a, b = [], []
    for _ in range(opt["runs"]):
        dt, x = chained(); a.append(dt * 1e3)
        dt, y = two_calls(); b.append(dt * 1e3)
        assert x == y, "the chained call and the two calls disagree"
    lines.append({"part": "chained", "genes": G, "taxa": n, "cols": m + m // 4, "kept_columns": x[2], "genes_kept": sum(x[0]),
                  "chained_wall_ms": a, "two_calls_wall_ms": b})
    print(json.dumps(lines[-1]), flush=True)
    if opt["out"]:
        with open(opt["out"], "w") as f:
            f.write("\n".join(json.dumps(x) for x in lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main(sys.argv[1:])
