#!/usr/bin/env python
"""Times the MinHash path on the device ("MinHash kernels").

usage: measure_mash.py [--ingroup 12] [--pool 500] [--bases 3000000] [--k 21] [--s 100000] [--repeats 3] [--baseline 64] [--seed 1] [--out FILE]
The genomes are copies of one random genome of --bases bases with substitutions at rates from 0.5 % to 20 %, seeded, one record
each.  A context with cfg.profile = 1; one warm-up call on four other genomes; then --repeats times pml_mash_distances(ingroup,
pool): pml_mash_stats' HIP-event times of the upload, k_mash_hash, the selection (k_mash_cut, k_mash_compact, the sort, k_mash_unique)
and k_mash_pairs, the repeats of the cut, and the host clock around the call.  Then, on the first --baseline genomes and alternating
--repeats times, pml_mash_sketch with the histogram cut and with pml_debug_mash_full_sort (every value sorted): the one comparison
there is.  Bytes of k_mash_hash: one read per byte and one 8-byte value written per byte, against 8 TB/s (spec) and 6.3 TB/s
(achievable) of HBM.  Prints one JSON line."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pepr_amd import engine

BASES = np.frombuffer(b"ACGT", dtype=np.uint8)


def family(rng, count, n):
    base = rng.integers(0, 4, n, dtype=np.uint8)
    out = []
    for g in range(count):
        rate = 0.005 + 0.195 * g / max(count - 1, 1)
        a = base.copy()
        pos = rng.integers(0, n, int(rate * n))
        a[pos] = (a[pos] + rng.integers(1, 4, pos.size, dtype=np.uint8)) & 3
        out.append([BASES[a].tobytes()])
    return out


def delta(a, b):
    return {k: b[k] - a[k] for k in a}


def main(argv):
    opt = {"ingroup": 12, "pool": 500, "bases": 3000000, "k": 21, "s": 100000, "repeats": 3, "baseline": 64, "seed": 1, "out": ""}
    for i in range(0, len(argv) - 1, 2):
        key = argv[i].lstrip("-")
        opt[key] = type(opt[key])(argv[i + 1])
    rng = np.random.default_rng(opt["seed"])
    k, s, n = opt["k"], opt["s"], opt["bases"]
    ctx = engine.Context(0, profile=True)
    warm = family(rng, 4, n)
    ctx.mash_distances(warm[:2], warm[2:], k, s)
    ctx.debug_mash_full_sort(True)
    ctx.mash_sketch(warm[:2], k, s)
    ctx.debug_mash_full_sort(False)
    genomes = family(rng, opt["ingroup"] + opt["pool"], n)
    rng.shuffle(genomes)
    ingroup, pool = genomes[:opt["ingroup"]], genomes[opt["ingroup"]:]
    G = len(genomes)
    windows = G * (n - k + 1)
    runs = []
    for _ in range(opt["repeats"]):
        before = ctx.mash_stats()
        t0 = time.perf_counter()
        r = ctx.mash_distances(ingroup, pool, k, s)
        wall = time.perf_counter() - t0
        d = delta(before, ctx.mash_stats())
        d["wall_ms"] = wall * 1e3
        runs.append(d)
    best = {key: min(x[key] for x in runs) for key in ("upload_ms", "hash_ms", "select_ms", "pairs_ms", "wall_ms")}
    hash_bytes = G * (n + 1) * 9.0
    pairs = len(ingroup) * len(pool)
    line = {"ingroup": len(ingroup), "pool": len(pool), "bases": n, "k": k, "s": s, "windows": windows, "runs": runs, "best": best,
            "cut_repeats_per_call": [x["repeats"] for x in runs],
            "k_mash_hash_windows_per_s": windows / best["hash_ms"] * 1e3 if best["hash_ms"] else None,
            "k_mash_hash_bytes": hash_bytes, "k_mash_hash_TBps": hash_bytes / best["hash_ms"] / 1e9 if best["hash_ms"] else None,
            "k_mash_hash_share_of_8TBps": hash_bytes / best["hash_ms"] / 1e9 / 8.0 if best["hash_ms"] else None,
            "k_mash_hash_share_of_6.3TBps": hash_bytes / best["hash_ms"] / 1e9 / 6.3 if best["hash_ms"] else None,
            "k_mash_pairs_per_s": pairs / best["pairs_ms"] * 1e3 if best["pairs_ms"] else None,
            "distance_range": [float(r["distance"].min()), float(r["distance"].max())],
            "mean_common": float(r["common"].mean())}
    nb = min(opt["baseline"], G)
    if nb > 0:
        sub = genomes[:nb]
        cut_ms, full_ms, same = [], [], True
        for _ in range(opt["repeats"]):
            a = ctx.mash_stats()
            sk = ctx.mash_sketch(sub, k, s)
            b = ctx.mash_stats()
            ctx.debug_mash_full_sort(True)
            sk_full = ctx.mash_sketch(sub, k, s)
            ctx.debug_mash_full_sort(False)
            c = ctx.mash_stats()
            cut_ms.append(b["select_ms"] - a["select_ms"])
            full_ms.append(c["select_ms"] - b["select_ms"])
            same = same and all((x == y).all() for x, y in zip(sk, sk_full))
        line.update({"baseline_genomes": nb, "select_ms_histogram_cut": cut_ms, "select_ms_full_sort": full_ms, "baseline_same_sketches": same})
    print(json.dumps(line), flush=True)
    if opt["out"]:
        with open(opt["out"], "w") as f:
            f.write(json.dumps(line) + "\n")
    ctx.close()


if __name__ == "__main__":
    main(sys.argv[1:])
