#!/usr/bin/env python
"""Wall time of the column bootstrap: pml_bootstrap (host draws, resampled text, one alignment) against pml_bootstrap2 (replicates
built on the device from resident genes), ML, same replicate count and epsilon (DESIGN.md 9 names the run).

usage: python tools/measure_bootstrap.py [--reps 100] [--runs 3] [--genes 1,20] [--taxa 50] [--sites 1000]
For every gene count G: one alignment of --taxa x (G * --sites) columns simulated on one tree, cut into G genes.  pml_bootstrap gets
the concatenated text, pml_bootstrap2 the genes.  One warm-up call of each (2 replicates), then --runs alternated timed calls of
each; every time is printed, nothing is averaged away.  The replicate-build share: for pml_bootstrap2 the deltas of pml_boot_stats
(profile mode: HIP-event times of the four kernels, and the host wall time from the count launch to the NJ starts); for
pml_bootstrap one extra call under PML_TRACE whose stderr gives the replicates' encode + NJ-start time and the arena allocation +
upload time (the resampling of the text itself is not separately timed there, so that figure is a lower bound).
Prints one JSON line per gene count."""
import json
import os
import re
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pepr_amd import engine, synth


def _stderr_of(fn):
    """fn() with the process's fd 2 (where the library's PML_TRACE lines go) captured -> (result, text)"""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as f:
        os.dup2(f.fileno(), 2)
        try:
            r = fn()
        finally:
            os.dup2(saved, 2); os.close(saved)
        f.seek(0)
        return r, f.read().decode(errors="replace")


def main(argv):
    opt = {"reps": 100, "runs": 3, "genes": "1,20", "taxa": 50, "sites": 1000, "seed": 7}
    for i in range(0, len(argv) - 1, 2):
        opt[argv[i].lstrip("-")] = argv[i + 1]
    reps, runs, taxa, sites, seed = (int(opt[k]) for k in ("reps", "runs", "taxa", "sites", "seed"))
    ctx = engine.Context(0, profile=True)
    for G in [int(x) for x in str(opt["genes"]).split(",")]:
        names, rows, _ = synth.simulate_alignment(taxa, G * sites, 9000 + G)
        genes = [(names, [r[g * sites:(g + 1) * sites] for r in rows]) for g in range(G)]
        kw = dict(seed=seed, spr_radius=5, epsilon=1e-3)
        ctx.bootstrap((names, rows), reps=2, **kw); ctx.bootstrap2(genes, reps=2, **kw)                 # warm-up
        out = {"genes": G, "taxa": taxa, "columns": G * sites, "reps": reps, "bootstrap_s": [], "bootstrap2_s": [], "build_ms": [], "kernel_ms": []}
        for _ in range(runs):
            t0 = time.perf_counter(); a = ctx.bootstrap((names, rows), reps=reps, **kw); out["bootstrap_s"].append(round(time.perf_counter() - t0, 3))
            s0 = ctx.boot_stats()
            t0 = time.perf_counter(); b = ctx.bootstrap2(genes, reps=reps, **kw); out["bootstrap2_s"].append(round(time.perf_counter() - t0, 3))
            s1 = ctx.boot_stats()
            out["build_ms"].append(round(s1["build_ms"] - s0["build_ms"], 3))
            out["kernel_ms"].append({k: round(s1["ms"][k] - s0["ms"][k], 4) for k in s1["ms"]})
            out["launches"] = {k: s1["launches"][k] - s0["launches"][k] for k in s1["launches"]}
        out["lnl"] = [a["lnl"], b["lnl"]]
        out["rf_best"] = engine.rf_distance(re.sub(r"\)\d+:", "):", a["newick"]), re.sub(r"\)\d+:", "):", b["newick"]))
        os.environ["PML_TRACE"] = "1"
        try:
            _, err = _stderr_of(lambda: ctx.bootstrap((names, rows), reps=reps, **kw))
        finally:
            del os.environ["PML_TRACE"]
        enc = [float(x) for x in re.findall(r"create: encode \+ start trees of \d+ genes ([0-9.]+) ms", err)]
        lay = [float(x) for x in re.findall(r"layout: arena [0-9.]+ GiB allocated \+ uploaded in ([0-9.]+) ms", err)]
        # the first create / layout pair is the best tree's single alignment; the others are the replicate sub-batches
        out["bootstrap_replicate_encode_ms"] = round(sum(enc[1:]), 1)
        out["bootstrap_replicate_alloc_upload_ms"] = round(sum(lay[1:]), 1)
        out["bootstrap_sub_batches"] = max(len(enc) - 1, 0)
        print(json.dumps(out), flush=True)
    ctx.close()


if __name__ == "__main__":
    main(sys.argv[1:])
