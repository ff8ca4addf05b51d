#!/usr/bin/env python
"""Times the gene homoplasy test on the device ("Gene-steps kernels").

usage: measure_genesteps.py [--genes 500] [--taxa 200] [--cols 5000] [--reps 1000] [--runs 3] [--seed 1]
The genes are evolved down one random tree (8 % change per branch, 3 % gaps); the tree is that tree.  A context with cfg.profile = 1:
pml_gene_steps_stats' HIP-event times of k_fitch_sitesteps, k_steps_expand and k_colminsteps for one pml_gene_steps call (after a
warm-up call on two of the genes), then of k_steps_resample for `runs` pml_step_thresholds calls in each mode (steps beyond the
minimum, multiple 3; with and without replacement) next to the wall time of the call.  Prints one JSON line."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pepr_amd import engine


def evolved(rng, ngenes, ntax, ncols):
    letters = np.frombuffer(b"ARNDCQEGHILKMFPSTWYV", dtype=np.uint8)
    width = ngenes * ncols
    names = ["t%03d" % i for i in range(ntax)]
    nodes, nxt, children, text = list(range(ntax)), ntax, {}, {i: names[i] for i in range(ntax)}
    while len(nodes) > 1:
        i, j = sorted(rng.choice(len(nodes), 2, replace=False))
        children[nxt] = (nodes[i], nodes[j])
        text[nxt] = "(%s,%s)" % (text.pop(nodes[i]), text.pop(nodes[j]))
        nodes = [x for k, x in enumerate(nodes) if k not in (i, j)] + [nxt]
        nxt += 1
    root = nxt - 1
    seq = {root: rng.integers(0, 20, width, dtype=np.uint8)}
    rows = [None] * ntax
    stack = [root]
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
        else:
            row = letters[seq.pop(v)]
            row[rng.random(width) < 0.03] = ord("-")
            rows[v] = row
    genes = [(names, [rows[t][g * ncols:(g + 1) * ncols].tobytes() for t in range(ntax)]) for g in range(ngenes)]
    return genes, text[root] + ";"


def main(argv):
    a = {"genes": 500, "taxa": 200, "cols": 5000, "reps": 1000, "runs": 3, "seed": 1}
    for k in range(0, len(argv), 2):
        a[argv[k].lstrip("-")] = int(argv[k + 1])
    rng = np.random.default_rng(a["seed"])
    t0 = time.time()
    genes, tree = evolved(rng, a["genes"], a["taxa"], a["cols"])
    out = {"shape": a, "generate_s": round(time.time() - t0, 2)}
    ctx = engine.Context(0, profile=True)
    ctx.gene_steps(genes[:2], tree)                # warm-up: code objects loaded
    s0 = ctx.gene_steps_stats()
    t0 = time.time()
    r = ctx.gene_steps(genes, tree)
    out["gene_steps_wall_s"] = round(time.time() - t0, 3)
    s1 = ctx.gene_steps_stats()
    for k in ("fitch_sitesteps", "steps_expand", "colminsteps"):
        out[k + "_ms"] = round(s1[k + "_ms"] - s0[k + "_ms"], 4)
        out[k + "_launches"] = s1[k + "_launches"] - s0[k + "_launches"]
    out["columns"] = int(r["ncols"])
    out["total_steps"] = int(r["gene_steps"].sum())
    draws = int(r["ncols"]) * a["reps"]
    ctx.step_thresholds(r, engine.STEPS_BEYOND_MIN, True, 3, 8, 0.05, 1)         # warm-up
    ctx.step_thresholds(r, engine.STEPS_BEYOND_MIN, False, 3, 8, 0.05, 1)
    for replace in (True, False):
        key = "replace" if replace else "no_replace"
        out[key] = []
        for run in range(a["runs"]):
            s0 = ctx.gene_steps_stats()
            t0 = time.time()
            th = ctx.step_thresholds(r, engine.STEPS_BEYOND_MIN, replace, 3, a["reps"], 0.05, 1 + run)
            wall = time.time() - t0
            s1 = ctx.gene_steps_stats()
            ms = s1["steps_resample_ms"] - s0["steps_resample_ms"]
            out[key].append({"resample_ms": round(ms, 3), "table_ms": round(s1["steps_table_ms"] - s0["steps_table_ms"], 4), "wall_s": round(wall, 3),
                             "draws_per_s": round(draws / (ms * 1e-3), 0) if ms > 0 else None, "genes_over_threshold": int((r["gene_beyond"] > th["threshold"]).sum())})
    out["draws_per_call"] = draws
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main(sys.argv[1:])
