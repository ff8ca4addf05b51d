#!/usr/bin/env python
"""Times the multiple alignment's kernels (csrc/msa.hip) class by class and on a mixed workload, beside the host twin.

usage: measure_msa.py [--class-sets 4096] [--sets 1500] [--n 12] [--length 300] [--host-sets 6] [--seed 1]
Each class alone: --class-sets sets of two related proteins at the class's one-pass limit (the widest class also at three
passes): one level, one merge a set, the class chosen by length.  The mixed workload: --sets families of --n proteins around
--length residues (substitutions, a few deletions), the shape of a bundled example's selected sets.  Kernel times are HIP events
(profile mode: k_msa_colv, k_msa_dp, k_msa_walk, k_msa_gather, and the pair scores' k_sw_score), the calls are wall clock; the
first call of each shape warms up and is not counted.  The host twin: one thread over --host-sets of the mixed sets.  Prints
DP cells per second for all of them and the share of the kernels' time in DP, walk and gather.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pepr_amd import engine

LETTERS = np.frombuffer(b"ARNDCQEGHILKMFPSTWYV", dtype=np.uint8)


def family(rng, n, length, frac=0.15, deletions=2):
    root = rng.integers(0, 20, length)
    out = []
    for _ in range(n):
        s = root.copy()
        hit = rng.random(length) < frac
        s[hit] = rng.integers(0, 20, int(hit.sum()))
        for _ in range(int(rng.integers(0, deletions + 1))):
            at = int(rng.integers(0, max(len(s) - 8, 1)))
            s = np.delete(s, slice(at, at + int(rng.integers(1, 8))))
        out.append(LETTERS[s].tobytes().decode())
    return out


def measured(ctx, sets):
    a, sa = ctx.msa_stats(), ctx.sw_stats()
    t0 = time.perf_counter()
    ctx.msa_align(sets)
    wall = time.perf_counter() - t0
    b, sb = ctx.msa_stats(), ctx.sw_stats()
    ms = [y - x for x, y in zip(a["ms"], b["ms"])]
    return {"cells": b["cells"] - a["cells"], "ms": ms, "wall": wall, "levels": b["levels"] - a["levels"], "merges": b["merges"] - a["merges"],
            "sw_ms": sum(sb["class_ms"]) - sum(sa["class_ms"]), "sw_cells": sb["cells"] - sa["cells"]}


def report(what, m):
    k = sum(m["ms"])
    print("%s: %d merges in %d levels, %.3e cells; k_msa_dp %.3f ms = %.3e cells/s; colv %.3f, walk %.3f, gather %.3f ms (DP %.0f%%, walk %.0f%%, gather %.0f%% of the "
          "four); k_sw_score %.3f ms for %.3e cells; the call %.3f s = %.3e cells/s"
          % (what, m["merges"], m["levels"], m["cells"], m["ms"][1], m["cells"] / (m["ms"][1] * 1e-3), m["ms"][0], m["ms"][2], m["ms"][3],
             100 * m["ms"][1] / k, 100 * m["ms"][2] / k, 100 * m["ms"][3] / k, m["sw_ms"], m["sw_cells"], m["wall"], m["cells"] / m["wall"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--class-sets", type=int, default=4096)
    ap.add_argument("--sets", type=int, default=1500)
    ap.add_argument("--n", type=int, default=12)
    ap.add_argument("--length", type=int, default=300)
    ap.add_argument("--host-sets", type=int, default=6)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    ctx = engine.Context(0, profile=True)
    lim = engine.msa_limits()
    for cls, rows in list(enumerate(lim["rows"])) + [(2, 3 * lim["rows"][2])]:
        sets = [family(rng, 2, rows, deletions=0) for _ in range(a.class_sets)]
        ctx.msa_align(sets[:4])
        report("class %d (%2d lanes), X and Y of %4d columns" % (cls, lim["lanes"][cls], rows), measured(ctx, sets))
    sets = [family(rng, a.n, int(np.clip(np.exp(rng.normal(np.log(a.length), 0.3)), 40, 2000))) for _ in range(a.sets)]
    ctx.msa_align(sets[:4])
    m = measured(ctx, sets)
    report("mixed workload, %d sets of %d proteins around %d residues" % (a.sets, a.n, a.length), m)
    sample = sets[:a.host_sets]
    t0 = time.perf_counter()
    h = engine.msa_align_host(sample)
    hw = time.perf_counter() - t0
    before = ctx.msa_stats()["cells"]
    assert ctx.msa_align(sample) == h
    hcells = ctx.msa_stats()["cells"] - before
    print("host twin, one thread, %d of the sets (pair scores included): %.3e cells in %.3f s = %.3e cells/s; device call / host = %.1f"
          % (len(sample), hcells, hw, hcells / hw, (m["cells"] / m["wall"]) / (hcells / hw)))
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
