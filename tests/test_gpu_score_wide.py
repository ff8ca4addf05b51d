"""The wide scoring kernel (k_oplist_wide: 512-thread workgroups, tip tables of one cherry / pitchfork side in LDS) against the
256-thread scoring kernel it replaces for chained launches (PML_CHAIN_VARIANT=11 selects the old one): bit for bit, and both
against the f64 oracle.  The switch is read once per process, so each choice runs tests/wide_harness.py in its own process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import wide_harness

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(variant):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), os.environ.get("PYTHONPATH", "")]))
    env.pop("PML_CHAIN_VARIANT", None)
    if variant is not None:
        env["PML_CHAIN_VARIANT"] = str(variant)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "wide_harness.py")], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads(p.stdout)


@pytest.fixture(scope="module")
def runs():
    return _run(None), _run(11)


def test_wide_kernel_is_bit_identical_to_the_256_thread_kernel(runs):
    wide, narrow = runs
    assert wide.keys() == narrow.keys() == wide_harness.cases().keys()
    for name in wide:
        assert wide[name] == narrow[name], name
        w = wide[name]
        assert w["score"] == w["replay"] == w["stored"] and w["score_site"] == w["replay_site"] == w["stored_site"], name
    # one chunk, exactly one 256-pattern workgroup, one pattern more, and a gene of the benchmark's shape
    npat = wide["sizes"]["npat"]
    assert npat[0] <= 32 and npat[1] == 256 and npat[2] == 257 and npat[3] > 768, npat
    # the codes of the two genes differ, hence their likelihoods
    assert wide["plain_codes"]["score"] != wide["gaps_and_ambiguity"]["score"]


def test_wide_kernel_against_the_oracle(runs, oracle_lib):
    import test_gpu_models as tm
    po = oracle_lib
    wide, _ = runs
    for name, (genes, newicks, alpha, mseed) in wide_harness.cases().items():
        model = po.Model(0) if mseed is None else tm.oracle_model(po, *tm.random_matrix(mseed))
        for i, ((names, rows), nw) in enumerate(zip(genes, newicks)):
            a = po.Alignment(names, rows)
            ref, refs = po.Engine(a, model, 4, alpha).site_lnl(po.Tree(nw, a))
            got = np.array([float.fromhex(x) for x in wide[name]["score_site"][i]])
            assert abs(float.fromhex(wide[name]["score"][i]) - ref) < 1e-9 * abs(ref), (name, i)
            assert np.abs(got - refs).max() < 1e-9, (name, i)
