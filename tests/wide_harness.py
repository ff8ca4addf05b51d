"""Scores a fixed set of batches through recorded scoring plans and prints the per-site lnL (float.hex JSON);
tests/test_gpu_score_wide.py runs it once per PML_CHAIN_VARIANT (the switch is read once per process) and compares the outputs
bit for bit.  cases() is imported by the test for the oracle side."""
import json
import sys

import numpy as np

from pepr_amd import synth


def _first_patterns(names, rows, n):
    """the alignment cut down to the first n distinct columns (one site per pattern)"""
    cols, seen = [], set()
    for j in range(len(rows[0])):
        c = "".join(r[j] for r in rows)
        if c not in seen:
            seen.add(c); cols.append(j)
        if len(cols) == n:
            break
    assert len(cols) == n
    return names, ["".join(r[j] for j in cols) for r in rows]


def _with_codes(rows, seed, frac):
    """gaps, X, B and Z sprinkled over every row: cherries and pitchforks whose tips are not plain amino acids"""
    rng = np.random.default_rng(seed)
    out = []
    for r in rows:
        a = np.array(list(r))
        hit = rng.random(a.size) < frac
        a[hit] = rng.choice(list("-XBZ"), int(hit.sum()))
        out.append("".join(a))
    return out


# both children of the node next to t0 are pitchforks: ((a,b),c) x ((d,e),f)
PITCH2 = "(t0:0.11,(((t1:0.2,t2:0.13):0.07,t3:0.3):0.09,((t4:0.05,t5:0.21):0.12,t6:0.17):0.08):0.1);"


def cases():
    """name -> (genes [(names, rows)], newicks, alpha, matrix seed or None); every batch holds a gene of more than 128 patterns"""
    out = {}
    big = synth.simulate_alignment(50, 1000, 4242, 0.8)
    n20 = synth.simulate_alignment(20, 700, 77, 0.8)
    one = synth.simulate_alignment(9, 30, 5, 0.8)
    sizes = [(one[0], one[1]), _first_patterns(n20[0], n20[1], 256), _first_patterns(n20[0], n20[1], 257), (big[0], big[1])]
    out["sizes"] = (sizes, [one[2], n20[2], n20[2], big[2]], 0.8, None)
    g = synth.simulate_alignment(40, 600, 31, 0.8)
    out["plain_codes"] = ([(g[0], g[1])], [g[2]], 0.7, None)
    out["gaps_and_ambiguity"] = ([(g[0], _with_codes(g[1], 9, 0.15))], [g[2]], 0.7, None)
    p = synth.simulate_alignment(7, 400, 12, 0.8)
    out["pitch_x_pitch"] = ([(p[0], p[1]), (p[0], _with_codes(p[1], 3, 0.1))], [PITCH2, PITCH2], 0.9, None)
    out["other_matrix"] = ([(g[0], g[1]), (g[0], _with_codes(g[1], 10, 0.1))], [g[2], g[2]], 0.6, 23)
    return out


def main():
    import test_gpu_models as tm
    from pepr_amd import engine
    ctx = engine.Context(0)
    out = {}
    for name, (genes, newicks, alpha, mseed) in cases().items():
        b = engine.Batch(ctx, genes, newicks, alpha=alpha)
        if mseed is not None:
            b.set_matrix(*tm.random_matrix(mseed))
        rec = {"npat": [int(x) for x in b.npatterns()]}
        for leg, stored in (("score", False), ("replay", False), ("stored", True)):
            lnl = b.score(stored=stored)
            rec[leg] = [float(x).hex() for x in lnl]
            rec[leg + "_site"] = [[float(x).hex() for x in b.site_lnl(i, len(genes[i][1][0]))] for i in range(len(genes))]
        b.close()
        out[name] = rec
    ctx.close()
    json.dump(out, sys.stdout)


if __name__ == "__main__":
    main()
