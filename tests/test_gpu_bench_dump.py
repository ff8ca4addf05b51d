"""bench.py --dump-outputs: the per-gene lnL of the last timed step, written as .npy, is the same from run to run (seeded
genes) and is the likelihood of those genes (CPU oracle); --steps sets the number of timed passes.  bench.py runs in its
own process, as the driver runs it."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from pepr_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(steps, out_dir):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "tiny", "--steps", str(steps), "--warmup", "1",
                        "--no-cpu-baseline", "--no-search", "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    line, = [l for l in p.stdout.splitlines() if l.startswith("{")]
    return json.loads(line)


def test_dump_outputs_repeat_and_match_the_oracle(tmp_path, oracle_lib):
    po = oracle_lib
    a, b = tmp_path / "a", tmp_path / "b"
    ja, jb = _bench(2, a), _bench(5, b)
    for j, steps in ((ja, 2), (jb, 5)):
        # one k_oplist launch per pass of the one resident sub-batch: launches of the timed region = ms per step x steps / ms per launch
        assert j["steps"] == steps and round(j["kernels_ms_per_step"]["newview"] * steps / j["roofline"]["avg_launch_ms"]) == steps
    assert sorted(os.listdir(a)) == sorted(os.listdir(b)) == ["lnl.npy", "stored_lnl.npy"]
    la, lb = np.load(a / "lnl.npy"), np.load(b / "lnl.npy")
    assert la.dtype == np.float64 and la.shape == (8,)
    assert np.array_equal(la, lb) and np.array_equal(la, np.load(a / "stored_lnl.npy")) and np.array_equal(la, np.load(b / "stored_lnl.npy"))
    for g in range(8):                               # bench.py's genes: seed = 1 + gene id, alpha 0.8
        names, rows, nw = synth.simulate_alignment(12, 200, 1 + g, 0.8)
        al = po.Alignment(names, rows)
        ref = po.Engine(al, po.Model(0), 4, 0.8).lnl(po.Tree(nw, al))
        assert abs(la[g] - ref) < 1e-9 * abs(ref), (g, la[g], ref)
