#!/usr/bin/env python
"""What RAxML's schedule (pml_search2) buys over the fixed-radius search, on the bench's genes.

Genes: the C3 set of bench.py (50 taxa x 1000 sites, seeds 1..128) and a C4-shaped handful (200 taxa x 5000 sites).  Settings:
  1. pml_search, radius 5 (what the shim and the mirror run today)
  2. pml_search2, fixed radius 10
  3. pml_search2, radius determined on the start tree
  4. the same plus the thorough phase, thorough_top 1, 3 and 0 (= all)
every one from the parsimony start of seed 12345, as `raxmlHPC -f d -p 12345`.  Per setting: wall time of the call, the number
of genes more than 1e-3 lnL below the optimised generating tree and the worst deficit, the mean RF distance to the
generating tree, and the distribution of the chosen radii.  One JSON document on stdout / --out; no thresholds.

    python tools/search_schedule_eval.py --genes 128 --c4-genes 0 --out profiles/search_schedule_eval_c3.json
    python tools/search_schedule_eval.py --genes 0 --c4-genes 4 --tops 3 --out profiles/search_schedule_eval_c4.json
"""
import argparse
import collections
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np                                          # noqa: E402

from pepr_amd import engine, synth                          # noqa: E402


def evaluate(ctx, genes, name, call, ref_lnl, report):
    t0 = time.perf_counter()
    out = call()
    wall = time.perf_counter() - t0
    res, traces = out if isinstance(out, tuple) else (out, None)
    deficit = np.array([ref_lnl[i] - r["lnl"] for i, r in enumerate(res)])
    rec = {"setting": name, "genes": len(genes), "wall_seconds": wall,
           "genes_below_generating_tree_by_1e-3": int((deficit > 1e-3).sum()), "worst_deficit_lnl": float(deficit.max()),
           "mean_lnl_minus_generating": float(-deficit.mean()),
           "mean_rf_to_generating_tree": float(np.mean([engine.rf_distance(g[2], r["newick"]) for g, r in zip(genes, res)]))}
    if traces is not None:
        rec["radius_chosen"] = dict(sorted(collections.Counter(t["radius_chosen"] for t in traces).items()))
        rec["accepted_steps_by_phase"] = dict(sorted(collections.Counter(s["phase"] for t in traces for s in t["steps"]).items()))
    report.append(rec)
    print(json.dumps(rec), file=sys.stderr, flush=True)


def run_set(ctx, label, genes, seed, tops, report):
    G = [(g[0], g[1]) for g in genes]
    ref = [r["lnl"] for r in ctx.optimize(G, [g[2] for g in genes], epsilon=1e-3)]       # the optimised generating trees
    common = dict(epsilon=1e-3, seed=seed)
    settings = [("pml_search radius 5", lambda: ctx.search(G, None, nni=True, spr_radius=5, **common)),
                ("search2 fixed 10", lambda: ctx.search2(G, None, radius=10, trace=True, **common)),
                ("search2 auto", lambda: ctx.search2(G, None, radius="auto", trace=True, **common))]
    for top in tops:
        settings.append(("search2 auto + thorough top %d" % top,
                         lambda top=top: ctx.search2(G, None, radius="auto", thorough=True, thorough_top=top, trace=True, **common)))
    ctx.search(G[:2], None, nni=True, spr_radius=5, **common)          # first use of the parsimony and search kernels
    for name, call in settings:
        evaluate(ctx, genes, label + ": " + name, call, ref, report)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--genes", type=int, default=128, help="C3 genes (seeds 1..N); 0 skips them")
    ap.add_argument("--c4-genes", type=int, default=4, help="C4-shaped genes (200 x 5000); 0 skips them")
    ap.add_argument("--tops", default="1,3,0", help="thorough_top values")
    ap.add_argument("--seed", type=int, default=12345)
    ap.add_argument("--out")
    args = ap.parse_args()
    tops = [int(x) for x in args.tops.split(",") if x != ""]
    ctx = engine.Context(0)
    report = []
    if args.genes:
        run_set(ctx, "C3", synth.simulate_genes(args.genes, 50, 1000, 1), args.seed, tops, report)
    if args.c4_genes:
        run_set(ctx, "C4 shape", synth.simulate_genes(args.c4_genes, 200, 5000, 1), args.seed, tops, report)
    ctx.close()
    doc = json.dumps({"tool": "tools/search_schedule_eval.py", "args": vars(args), "settings": report}, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(doc + "\n")
    print(doc)


if __name__ == "__main__":
    main()
