"""The host path of a replayed scoring step (Batch::replay_plan) and the two traversals it launches.

(a) A replay refreshes a gene's requests when its tree's length stamp or its rates epoch moved, not by comparing the lengths as
    bytes.  Every public call that writes branch lengths -- optimise, a search whose NNIs are accepted or undone, a search that
    replaces the tree -- and set_alpha must reach the next replay: its lnL equals, bit for bit, that of a fresh batch built from
    the same trees.  PML_CHECK_LEN_STAMP=1 keeps the byte compare running beside the stamps and fails the call if they disagree.
(b) In a profiling context every replay adds exactly one timed launch of each of its three kernels to kernel_stats(), and
    reading the statistics changes nothing.
(c) The register-resident and the stored traversal, wide and 256-thread kernel, at the smallest tile occupancies and tree shapes
    that matter (tests/step_path_harness.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import step_path_harness
from pepr_amd import engine, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fresh_scores(ctx, genes, batch, alphas):
    """the trees and rates of `batch` in a new batch: first score (no plan yet) and its replay"""
    newicks = [batch.newick(g, 30) for g in range(len(genes))]     # 30 decimals: every length >= 1e-6 reads back as the same double
    f = engine.Batch(ctx, genes, newicks, alpha=1.0)
    for g, a in enumerate(alphas):
        f.set_alpha(float(a), g)
    first, replay = f.score(), f.score()
    f.close()
    assert np.array_equal(first, replay)
    return first


def test_every_length_writer_reaches_the_replay(gpu_ctx, monkeypatch):
    monkeypatch.setenv("PML_CHECK_LEN_STAMP", "1")          # read when a plan is recorded
    sims = [synth.simulate_alignment(8, 200, 900 + i) for i in range(3)]
    genes = [(s[0], s[1]) for s in sims]
    # start trees that are not the simulated ones, so that the search has NNIs to accept: every gene gets its neighbour's tree
    starts = [sims[(i + 1) % 3][2] for i in range(3)]
    b = engine.Batch(gpu_ctx, genes, starts, alpha=0.8)
    alphas = [0.8] * 3
    first = b.score()                                       # records the plan
    assert np.array_equal(b.score(), first)
    assert np.array_equal(first, _fresh_scores(gpu_ctx, genes, b, alphas))
    # set: one gene's rates
    b.set_alpha(0.5, 1); alphas[1] = 0.5
    one = b.score()
    assert one[1] != first[1] and one[0] == first[0] and one[2] == first[2]
    assert np.array_equal(one, _fresh_scores(gpu_ctx, genes, b, alphas))
    # optimise: every gene's lengths move under an unchanged topology, so the next score is a replay of the recorded plan
    _, al = b.optimize(optimize_alpha=False)
    assert np.array_equal(al, alphas)
    opt = b.score()
    assert np.all(opt > one) and np.array_equal(b.score(), opt)
    assert np.array_equal(opt, _fresh_scores(gpu_ctx, genes, b, alphas))
    # a search with NNIs: accepted moves, rejected ones undone from a backup copy (which carries its stamp back)
    before = [b.newick(g, -1) for g in range(3)]
    _, al = b.search(optimize_alpha=False, nni=True)
    assert any(engine.rf_distance(before[g], b.newick(g, -1)) > 0 for g in range(3)), "no NNI was accepted: the case tests nothing"
    nni = b.score()
    assert np.all(nni >= opt) and np.array_equal(b.score(), nni)
    assert np.array_equal(nni, _fresh_scores(gpu_ctx, genes, b, alphas))
    # lengths again on the new topology: the plan recorded after the search is replayed with moved lengths
    b.optimize(optimize_alpha=False)
    again = b.score()
    assert np.array_equal(b.score(), again) and np.array_equal(again, _fresh_scores(gpu_ctx, genes, b, alphas))
    # tree replacement: a constraint the current tree of gene 0 cannot display makes the search start from a new tree
    names = genes[0][0]
    trees = [b.newick(g, -1) for g in range(3)]
    i, j = next((i, j) for i in range(1, 8) for j in range(i + 1, 8) if not any(_cherry(t, names[i], names[j]) for t in trees))
    cons = (sorted(names), ["1" if n in (names[i], names[j]) else "0" for n in sorted(names)])      # one column: the split ti tj | rest
    b.search(optimize_alpha=False, nni=True, constraints=cons)
    assert all(_cherry(b.newick(g, -1), names[i], names[j]) for g in range(3))
    rep = b.score()
    assert np.array_equal(b.score(), rep) and np.array_equal(rep, _fresh_scores(gpu_ctx, genes, b, alphas))
    b.close()


def _cherry(newick, a, c):
    """whether tips a and c (neither is the tip the text is rooted at) are a cherry of the tree (topology-only Newick text)"""
    return ("(%s,%s)" % (a, c)) in newick or ("(%s,%s)" % (c, a)) in newick


def test_replay_launch_statistics():
    ctx = engine.Context(0, profile=True)
    sims = [synth.simulate_alignment(8, 200, 910 + i) for i in range(3)]
    b = engine.Batch(ctx, [(s[0], s[1]) for s in sims], [s[2] for s in sims], alpha=0.8)
    first = b.score()                       # records the plan
    ctx.kernel_stats(reset=True)
    n = 5
    for _ in range(n):
        assert np.array_equal(b.score(), first)
    st = ctx.kernel_stats()
    for k in ("pmat", "newview", "reduce"):
        assert st[k]["launches"] == n and st[k]["ms"] > 0, (k, st[k])
    assert st["host_build"]["launches"] == n and st["host_wait"]["launches"] == n
    assert ctx.kernel_stats() == st
    # a reset between two replays: nothing of the old launches arrives afterwards
    b.score()
    ctx.kernel_stats(reset=True)
    z = ctx.kernel_stats()
    assert all(z[k]["launches"] == 0 and z[k]["ms"] == 0 for k in ("pmat", "newview", "reduce"))
    b.score()
    b.close()
    ctx.close()


def _run(variant):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), os.environ.get("PYTHONPATH", "")]))
    env.pop("PML_CHAIN_VARIANT", None)
    if variant is not None:
        env["PML_CHAIN_VARIANT"] = str(variant)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "step_path_harness.py")], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads(p.stdout)


@pytest.fixture(scope="module")
def runs():
    return _run(None), _run(11)


def test_stored_and_register_resident_passes_agree(runs):
    wide, narrow = runs
    assert wide.keys() == narrow.keys() == step_path_harness.NPAT.keys()
    for name, w in wide.items():
        assert w["score"] == w["replay"] == w["stored"] and w["score_site"] == w["replay_site"] == w["stored_site"], name
        assert w == narrow[name], name
        assert w["score"][0] != w["score"][1], name          # two trees over one alignment
    pad = lambda n: (n + 31) // 32 * 32
    assert [pad(wide[k]["npat"][0]) for k in ("one_chunk", "mpad_288", "mpad_544")] == [32, 288, 544]


def test_small_cases_against_the_oracle(runs, oracle_lib):
    po = oracle_lib
    wide, _ = runs
    for name, (genes, newicks, alpha, _) in step_path_harness.cases().items():
        for i, ((names, rows), nw) in enumerate(zip(genes, newicks)):
            a = po.Alignment(names, rows)
            ref, refs = po.Engine(a, po.Model(0), 4, alpha).site_lnl(po.Tree(nw, a))
            got = np.array([float.fromhex(x) for x in wide[name]["stored_site"][i]])
            assert abs(float.fromhex(wide[name]["stored"][i]) - ref) < 1e-9 * abs(ref), (name, i)
            assert np.abs(got - refs).max() < 1e-9, (name, i)
