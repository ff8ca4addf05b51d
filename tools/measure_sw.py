#!/usr/bin/env python
"""Times the homology search's kernel (csrc/sw.hip) class by class and on a mixed proteome set, beside the host twin.

usage: measure_sw.py [--genomes 3] [--proteins 400] [--class-queries 256] [--host-pairs 300] [--seed 1]
Each class alone: uniform queries at the class's one-pass limit (the widest class also at three passes) against one genome of
log-normal lengths, through the test door, timed by HIP events (profile mode); the first call of each shape warms up and is not
counted.  The mixed set: --genomes genomes of --proteins proteins, lengths log-normal around 300 (Aquificales is 12 x 1600-1800;
the fraction is printed), the whole call by wall clock and the kernels by events.  The host twin: one thread over a sample of the
same pairs.  Prints cells per second for all of them.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pepr_amd import engine

LETTERS = "ARNDCQEGHILKMFPSTWYV"


def protein(rng, n):
    return "".join(LETTERS[i] for i in rng.integers(0, 20, n))


def lengths(rng, n):
    return np.clip(np.exp(rng.normal(np.log(300.0), 0.55, n)).astype(int), 30, 3000)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genomes", type=int, default=3)
    ap.add_argument("--proteins", type=int, default=400)
    ap.add_argument("--class-queries", type=int, default=256)
    ap.add_argument("--host-pairs", type=int, default=300)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    ctx = engine.Context(0, profile=True)
    lim = engine.sw_class_limits()
    subjects = [protein(rng, n) for n in lengths(rng, a.proteins)]
    sres = sum(map(len, subjects))
    for cls, rows in list(enumerate(lim["rows"])) + [(2, 3 * lim["rows"][2])]:
        queries = [protein(rng, rows) for _ in range(a.class_queries)]
        ctx.debug_sw_scores(queries[:4], subjects[:8], force_class=cls)
        before = ctx.sw_stats()
        ctx.debug_sw_scores(queries, subjects, force_class=cls)
        after = ctx.sw_stats()
        ms = after["class_ms"][cls] - before["class_ms"][cls]
        cells = after["cells"] - before["cells"]
        print("class %d (%2d lanes) queries of %4d: %.3e cells in %8.3f ms = %.3e cells/s" % (cls, lim["lanes"][cls], rows, cells, ms, cells / (ms * 1e-3)))
    genomes = [[("g%d_p%d" % (g, i), protein(rng, n)) for i, n in enumerate(lengths(rng, a.proteins))] for g in range(a.genomes)]
    ctx.sw_search([g[:8] for g in genomes])
    before = ctx.sw_stats()
    t0 = time.perf_counter()
    r = ctx.sw_search(genomes)
    wall = time.perf_counter() - t0
    after = ctx.sw_stats()
    kms = sum(after["class_ms"]) - sum(before["class_ms"])
    print("mixed set %d x %d proteins (%.4f of Aquificales' cells): %.3e cells, %d hits; kernels %.3f ms = %.3e cells/s; the call %.3f s = %.3e cells/s"
          % (a.genomes, a.proteins, r["cells"] / 4e13, r["cells"], len(r["query"]), kms, r["cells"] / (kms * 1e-3), wall, r["cells"] / wall))
    flat = [p for g in genomes for p in g]
    sample = [flat[i] for i in rng.integers(0, len(flat), max(2, int(np.sqrt(a.host_pairs))))]
    t0 = time.perf_counter()
    h = engine.sw_search_host([sample])
    hw = time.perf_counter() - t0
    print("host twin, one thread, %d proteins of the set against each other: %.3e cells in %.3f s = %.3e cells/s; device / host = %.1f"
          % (len(sample), h["cells"], hw, h["cells"] / hw, (r["cells"] / wall) / (h["cells"] / hw)))
    print("one-genome subjects of the class runs: %d residues" % sres)
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
