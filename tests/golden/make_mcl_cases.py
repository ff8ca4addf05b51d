"""Writes tests/golden/mcl_cases.json: seeded weighted graphs as --abc text, clustered by an mcl binary (09-308, the one PEPR
bundles) given on the command line, with the lines it wrote.  A case is kept only if the binary, tests/mcl_ref.py in float64 and
tests/mcl_ref.py in float32 give the same lines; the number dropped is printed (more than one in ten means the rule is wrong,
not the cases).  Runs where the binary is; no test runs it.

    python tests/golden/make_mcl_cases.py /path/to/mcl
"""
import json
import os
import random
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import mcl_ref  # noqa: E402


def planted(rng, sizes, p_in, p_cross, one_way=0.3, repeats=0.1, selfs=0.1, isolated=0, bridge=True):
    """clusters of the given sizes; arcs inside with probability p_in (weights 50..400), across with p_cross (weights 20..120:
    the ranges overlap); a share of the arcs one-directional, repeated with another weight, or self hits"""
    n = sum(sizes)
    member = []
    for k, s in enumerate(sizes):
        member += [k] * s
    names = ["g%d|p%03d" % (member[i] % 7, i) for i in range(n)]
    order = list(range(n))
    rng.shuffle(order)
    lines = []

    def arc(a, b, w):
        lines.append("%s\t%s\t%s" % (names[a], names[b], w))
    for ia in range(n):
        for ib in range(ia + 1, n):
            a, b = order[ia], order[ib]
            same = member[a] == member[b]
            if not bridge and not same:
                continue
            if rng.random() < (p_in if same else p_cross):
                w = rng.randint(50, 400) if same else rng.randint(20, 120)
                w = w if rng.random() < 0.5 else round(w + rng.random(), 1)
                arc(a, b, w)
                if rng.random() >= one_way:
                    arc(b, a, w if rng.random() < 0.5 else rng.randint(20, 400))
                if rng.random() < repeats:
                    arc(a, b, rng.randint(20, 400))
    for i in range(n):
        if rng.random() < selfs:
            arc(i, i, rng.randint(100, 500))
    rng.shuffle(lines)
    for i in range(isolated):
        lines.insert(rng.randrange(len(lines) + 1), "lone%d\tlone%d\t%d" % (i, i, rng.randint(100, 500)))
    return "\n".join(lines) + "\n"


CASES = [
    # name, seed, inflation, sizes, p_in, p_cross, extras
    ("small_I1.5", 1, 1.5, [5, 4, 3], 0.9, 0.05, {}),
    ("small_I1.2", 2, 1.2, [6, 6, 5], 0.9, 0.04, {}),
    ("small_I2.0", 3, 2.0, [8, 7, 4, 2], 0.8, 0.06, {}),
    ("small_I3.0", 4, 3.0, [10, 9, 5], 0.7, 0.08, {}),
    ("equal_sizes", 5, 1.5, [6, 6, 6, 6, 3, 3], 0.9, 0.02, {}),
    ("isolated", 6, 1.5, [7, 5, 2], 0.9, 0.05, {"isolated": 3}),
    ("several_components", 7, 1.5, [12, 9, 9, 6, 4, 2, 2], 0.8, 0.0, {"bridge": False, "isolated": 2}),
    ("mid_I1.5", 8, 1.5, [20, 15, 15, 10, 6], 0.5, 0.03, {}),
    ("mid_I2.0", 9, 2.0, [25, 20, 12, 8], 0.45, 0.04, {}),
    ("noisy_I1.5", 10, 1.5, [18, 14, 14, 9], 0.6, 0.12, {}),
    ("wide_I1.2", 11, 1.2, [30, 25, 20, 15, 10], 0.4, 0.02, {}),
    ("wide_I3.0", 12, 3.0, [40, 30, 30, 20, 10], 0.35, 0.03, {}),
    ("wide_I1.5", 13, 1.5, [35, 35, 25, 20, 15], 0.35, 0.03, {"isolated": 0}),
]


def run_mcl(mcl, text, inflation):
    with tempfile.TemporaryDirectory() as d:
        f, o = os.path.join(d, "g.abc"), os.path.join(d, "g.out")
        with open(f, "w") as fh:
            fh.write(text)
        subprocess.run([mcl, f, "--abc", "-I", str(inflation), "-te", "1", "-o", o], check=True, capture_output=True)
        with open(o) as fh:
            return [ln for ln in fh.read().split("\n") if ln]


def main():
    mcl = sys.argv[1]
    kept, dropped = [], 0
    for name, seed, infl, sizes, p_in, p_cross, extra in CASES:
        text = planted(random.Random(seed), sizes, p_in, p_cross, **extra)
        lines = run_mcl(mcl, text, infl)
        r64 = mcl_ref.mcl_lines(text, np.float64, inflation=infl)
        r32 = mcl_ref.mcl_lines(text, np.float32, inflation=infl)
        n = len(mcl_ref.parse_abc(text)[0])
        ok = lines == r64 == r32
        print("%-20s n %3d  lines %2d  %s" % (name, n, len(lines), "kept" if ok else "DROPPED (ref64 %s, ref32 %s)" % (lines == r64, lines == r32)))
        if ok:
            kept.append({"name": name, "inflation": infl, "n": n, "abc": text, "lines": lines})
        else:
            dropped += 1
    print("dropped %d of %d" % (dropped, len(CASES)))
    with open(os.path.join(HERE, "mcl_cases.json"), "w") as fh:
        json.dump({"source": "mcl 09-308 --abc -I <inflation> -te 1", "cases": kept}, fh, indent=0)
        fh.write("\n")


if __name__ == "__main__":
    main()
