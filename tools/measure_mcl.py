#!/usr/bin/env python
"""Times the Markov clustering classes on a PEPR-shaped hit graph made from a seed: families of 10-20 members with noise arcs
(the packed and LDS classes) and a few components of several hundred to a few thousand nodes (the HBM class).  Prints the
device time per class from pml_mcl_stats (cfg.profile = 1) beside pml_mcl_cluster_host on the same graph, and checks that both
give the same clusters.

usage: measure_mcl.py [--seed 1] [--families 3000] [--mid 40] [--big 600 1500 3000] [--device 0]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pepr_amd import engine


def family(rng, first, size, p, arcs, lo=50, hi=400):
    for i in range(size):
        for j in range(i + 1, size):
            if rng.random() < p:
                arcs.append((first + i, first + j, float(rng.integers(lo, hi))))
    for i in range(1, size):                                    # connected: a chain under the random arcs
        arcs.append((first + i - 1, first + i, float(rng.integers(lo, hi))))


def graph(seed, families, mid, big):
    """(n, arcs): `families` components of 10-20 nodes, `mid` of 30-90, and one of every size in `big` made of planted families
    of 15-40 joined by weak arcs"""
    rng = np.random.default_rng(seed)
    arcs, n = [], 0
    for _ in range(families):
        s = int(rng.integers(10, 21))
        family(rng, n, s, 0.8, arcs)
        n += s
    for _ in range(mid):
        s = int(rng.integers(30, 91))
        family(rng, n, s, 0.3, arcs)
        n += s
    for s in big:
        at = n
        while at < n + s:
            m = min(int(rng.integers(15, 41)), n + s - at)
            family(rng, at, m, 0.6, arcs)
            if at > n:
                arcs.append((at - 1, at, float(rng.integers(20, 60))))
                for _ in range(3):
                    arcs.append((int(rng.integers(n, at)), int(rng.integers(at, at + m)), float(rng.integers(20, 60))))
            at += m
        n += s
    return n, arcs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--families", type=int, default=3000)
    ap.add_argument("--mid", type=int, default=40)
    ap.add_argument("--big", type=int, nargs="*", default=[600, 1500, 3000])
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    n, arcs = graph(a.seed, a.families, a.mid, a.big)
    print("graph: %d nodes, %d arcs, %d + %d + %d components" % (n, len(arcs), a.families, a.mid, len(a.big)))
    ctx = engine.Context(a.device, profile=True)
    ctx.mcl_cluster(40, [(i, i + 1, 1.0) for i in range(39)])                          # warm-up: module load, first launches
    s0 = ctx.mcl_stats()
    t0 = time.perf_counter()
    dev = ctx.mcl_cluster(n, arcs)
    t_dev = time.perf_counter() - t0
    s1 = ctx.mcl_stats()
    t0 = time.perf_counter()
    host = engine.mcl_cluster_host(n, arcs)
    t_host = time.perf_counter() - t0
    print("| stage | device ms |")
    print("|---|---|")
    for key, name in (("upload_fill_ms", "uploads and k_mcl_fill"), ("packed_ms", "packed class (n <= 16)"), ("lds_ms", "LDS class (n <= 96)"),
                      ("hbm_ms", "HBM class (host loop included)")):
        print("| %s | %.2f |" % (name, s1[key] - s0[key]))
    print("| the call, wall clock (front end and reading included) | %.2f |" % (t_dev * 1e3))
    print("| pml_mcl_cluster_host, wall clock | %.2f |" % (t_host * 1e3))
    print("launches: " + ", ".join("%s %d" % (k, s1[k] - s0[k]) for k in s1 if k.endswith("launches") or k == "sub_batches"))
    print("clusters: device %d, host %d, iterations %d / %d, %s" % (len(dev["clusters"]), len(host["clusters"]), dev["iterations"], host["iterations"],
                                                                    "equal" if dev["clusters"] == host["clusters"] else "DIFFERENT"))
    ctx.close()
    return 0 if dev["clusters"] == host["clusters"] else 1


if __name__ == "__main__":
    sys.exit(main())
