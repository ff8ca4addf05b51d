"""What a launch set costs, as the host accounts it: launches, bytes and flops of k_pmat, k_oplist and k_reduce for a recorded
and a replayed scoring pass (results kept in registers, and every CLV stored) and for a one-gene evaluation over cached CLVs.
A request that is no longer shared between the operations across one branch changes no result bit -- only k_pmat's work and
the upload grow -- so the figures are compared for exact equality (integers, and doubles the host adds up in a fixed order)
with tests/golden/launch_accounting.json, which holds what the commit before the launch builder was split out reports for
the same calls.  None of the calls has a Newton tail: other work on the device cannot change a count."""
import json
import os

import pytest

from pepr_amd import engine, synth

pytestmark = pytest.mark.gpu

SHAPES = [(5, 40), (9, 333), (16, 700), (33, 129), (50, 1000), (64, 2100)]      # the genes of tests/chain_harness.py
KINDS = ("pmat", "newview", "reduce")
FIGURES = ("launches", "algo_bytes", "algo_flops")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_accounting.json")


def measure():
    """{step: {kind: {figure: value}}} for the five steps, each taken from statistics reset before it"""
    ctx = engine.Context(0, profile=True)
    genes = [synth.simulate_alignment(nt, ns, 900 + i, missing_frac=0.1 * (i % 2)) for i, (nt, ns) in enumerate(SHAPES)]
    b = engine.Batch(ctx, [(g[0], g[1]) for g in genes], [g[2] for g in genes], alpha=0.8)
    steps = [("score_recorded", lambda: b.score()), ("score_replayed", lambda: b.score()),
             ("stored_recorded", lambda: b.score(stored=True)), ("stored_replayed", lambda: b.score(stored=True)),
             ("site_lnl_gene4", lambda: b.site_lnl(4, SHAPES[4][1]))]
    out = {}
    for name, call in steps:
        ctx.kernel_stats(reset=True)
        call()
        st = ctx.kernel_stats()
        out[name] = {k: {f: st[k][f] for f in FIGURES} for k in KINDS}
    b.close()
    ctx.close()
    return out


def test_launch_accounting_matches_recorded_figures():
    got = measure()
    with open(GOLDEN) as f:
        want = json.load(f)
    for step in got:
        print(step, json.dumps(got[step]))
    # a recorded pass and its replay are the same launch set
    assert got["score_recorded"] == got["score_replayed"]
    assert got["stored_recorded"] == got["stored_replayed"]
    # storing every CLV changes operation flags, not the transition-matrix requests (PFRAG * 8 bytes each)
    assert got["stored_recorded"]["pmat"] == got["score_recorded"]["pmat"]
    assert got["score_recorded"]["pmat"]["launches"] == 1 and got["score_recorded"]["pmat"]["algo_bytes"] > 0
    assert sorted(got) == sorted(want)
    for step in want:
        for kind in KINDS:
            for fig in FIGURES:
                assert got[step][kind][fig] == want[step][kind][fig], (step, kind, fig, got[step][kind][fig], want[step][kind][fig])
