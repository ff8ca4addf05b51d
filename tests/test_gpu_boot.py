"""pml_bootstrap2: the column bootstrap of a gene set with every replicate built on the device from the genes resident in HBM.
The four kernels alone against the restatement (boot_ref.py) and against the materialised text; the parsimony bootstrap against
the C oracle on that text, exactly; the ML bootstrap against the oracle's search; determinism, sub-batching, refusals."""
import collections
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import boot_ref as ref
import util
from pepr_amd import _lib, engine, synth
from test_gpu_jackknife import _encode_text, _sliced_genes
from test_gpu_jackknife3 import MASK, _genes, _leaves, _strip

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ML, PARSIMONY, PARSIMONY_BL = engine.TREE_ML, engine.TREE_PARSIMONY, engine.TREE_PARSIMONY_BL
REPS, SEED = 5, 3
EPS_GTR = 0.01          # as tests/test_gpu_jackknife2.py


def _boot_genes():
    """test_gpu_jackknife3's genes (37, 300, 257, 64, 5, 130 columns; genes that lack taxa; B / Z / X / - / ? residues) and a
    seventh of 1500 columns over the first 10 taxa, so that P exceeds twice k_boot_index's tile"""
    genes = _genes()
    names, rows, _ = synth.simulate_alignment(12, 1500, 4006)
    genes.append((names[:10], rows[:10]))
    return genes


GENES = _boot_genes()
FULL_SEED, REP_SEEDS = engine.jackknife_parsimony_seeds(SEED, REPS)
SELS = [[4], [2, 4], None]
KERNEL_REPS = [0, 1, 4]


def _labels_recount(newick, replicates, reps):
    """the percent labels a recount of the replicate trees gives for the tree's own bipartitions, sorted"""
    names = frozenset(_leaves(newick))
    rep_splits = [util.splits(t) for t in replicates]
    return sorted(int(0.5 + 100.0 * sum(s in rs or (names - s) in rs for rs in rep_splits) / reps)
                  for s in util.splits(_strip(newick)) if 1 < len(s) < len(names) - 1)


@pytest.fixture(scope="module")
def materialised():
    """the resampled text of (selection, replicate), built once and shared"""
    cache = {}

    def get(sel, rep, genes=GENES, seed=SEED):
        key = (None if sel is None else tuple(sel), rep, id(genes), seed)
        if key not in cache:
            cache[key] = ref.materialise(genes, sel, seed, rep)
        return cache[key]
    return get


# ---- 0. the conditions the cases below rely on, asserted, not tuned ----
def test_conditions():
    c2p, P = ref.col2pat(GENES)
    assert P > 2 * engine.boot_tile() and P > 256
    for r in range(REPS):
        cnt = ref.counts(GENES, None, SEED, r)
        print("replicate %d: P %d, npat %d, max count %d" % (r, P, int((cnt > 0).sum()), int(cnt.max())))
        assert cnt.max() >= 2 and (cnt > 0).sum() < P and cnt.sum() == len(c2p)


# ---- 1. the kernels alone ----
@pytest.mark.parametrize("rep", KERNEL_REPS)
@pytest.mark.parametrize("sel", SELS, ids=["gene4", "genes2+4", "all"])
def test_kernels_alone(gpu_ctx, materialised, sel, rep):
    before = gpu_ctx.boot_stats()["launches"]
    d = gpu_ctx.debug_boot_replicate(GENES, sel, SEED, rep, form=0)
    mid = gpu_ctx.boot_stats()["launches"]
    assert {k: mid[k] - before[k] for k in mid} == {"count": 1, "index": 1, "gather": 1, "pairs": 1}
    f = gpu_ctx.debug_boot_replicate(GENES, sel, SEED, rep, form=1)
    after = gpu_ctx.boot_stats()["launches"]
    assert {k: after[k] - mid[k] for k in mid} == {"count": 2, "index": 2, "gather": 2, "pairs": 1}     # form 1 builds both forms (peprml.h)
    c2p, P = ref.col2pat(GENES, sel)
    L = len(c2p)
    want = ref.counts(GENES, sel, SEED, rep)
    idx, npat, mpad = d["idx"], d["npat"], d["mpad"]
    # the compaction: strictly ascending, the restatement's
    assert len(idx) == npat and np.all(np.diff(idx) > 0) and np.array_equal(idx, ref.compact(want)) and npat < P
    assert mpad == (npat + 31) // 32 * 32 and d["cells"].shape == (len(d["names"]), mpad)
    # weights = counts, sum = L; padding = gap code, weight 0
    w = d["weights"]
    assert np.array_equal(w[:npat], want[idx].astype(np.float64)) and w.sum() == L and (w[:npat] > 0).all()
    assert not w[npat:].any() and np.all(d["cells"][:, npat:] == 22)
    # the code columns are the gathered selection's columns at idx
    gnames, codes, gw = gpu_ctx.debug_gather(GENES, sel)
    assert gnames == d["names"] and codes.shape[1] == P
    assert np.array_equal(d["cells"][:, :npat], codes[:, idx])
    # form 1: the same replicate as Fitch state sets with int weights; its padding is every state, weight 0 (mpad >= 32)
    assert f["names"] == d["names"] and f["npat"] == npat and np.array_equal(f["idx"], idx) and f["mpad"] == max(32, mpad)
    wantm = np.full(f["cells"].shape, 0xFFFFF, dtype=np.uint32)
    wantm[:, :npat] = MASK[codes[:, idx]]
    assert f["cells"].dtype == np.uint32 and np.array_equal(f["cells"], wantm)
    assert f["weights"].dtype == np.int32 and np.array_equal(f["weights"][:npat], want[idx]) and not f["weights"][npat:].any()
    # independent of any device encoder: {column -> number of draws} of the materialised text
    tnames, rows = materialised(sel, rep)
    assert tnames == d["names"] and len(rows[0]) == L
    enc = _encode_text(rows)
    text = collections.Counter(map(tuple, enc.T.tolist()))
    dev = collections.Counter()
    for q in range(npat):
        dev[tuple(d["cells"][:, q].tolist())] += int(w[q])
    assert dev == text
    # pair counts: a numpy count over the materialised text
    ok = enc < 20
    okp = (ok[:, None, :] & ok[None, :, :])
    cmp_ = okp.sum(axis=2)
    diff = (okp & (enc[:, None, :] != enc[None, :, :])).sum(axis=2)
    np.fill_diagonal(cmp_, 0); np.fill_diagonal(diff, 0)
    assert np.array_equal(d["cmp"], cmp_) and np.array_equal(d["diff"], diff)
    assert np.array_equal(f["cmp"], cmp_) and np.array_equal(f["diff"], diff)
    if sel == [4]:
        assert npat < 32
    if sel is None:
        assert P > 2 * engine.boot_tile() and want.max() >= 2 and any(len(g[0]) < len(d["names"]) for g in GENES)


def _wide_cases():
    """two inputs of more than 2 * BOOT_CHUNK columns, so that k_boot_count runs three workgroups per replicate, the last one
    partly filled: "lds" has few patterns (five residues over four taxa: P <= 625, the LDS histogram flushed with one global add
    per bin), "auto" has nearly one pattern per column (P > BOOT_LDS_BINS: the call switches to the global form by itself)"""
    rng = np.random.default_rng(20261020)
    four, six = ["w%d" % i for i in range(4)], ["v%d" % i for i in range(6)]
    return {"lds": [(four, ["".join(rng.choice(list("ACDE-"), 40001)) for _ in four])],
            "auto": [(six, ["".join(rng.choice(list(ref.AA), 36000)) for _ in six])]}


WIDE = _wide_cases()
WIDE_REPS = [0, 4]
_HPP = open(os.path.join(ROOT, "pepr_amd", "csrc", "boot.hpp")).read()
BOOT_CHUNK, BOOT_LDS_BINS = (int(re.search(r"constexpr int %s = (\d+);" % k, _HPP).group(1)) for k in ("BOOT_CHUNK", "BOOT_LDS_BINS"))


@pytest.mark.parametrize("rep", WIDE_REPS)
@pytest.mark.parametrize("case", sorted(WIDE))
def test_count_over_several_workgroups(gpu_ctx, case, rep):
    genes = WIDE[case]
    c2p, P = ref.col2pat(genes)
    L = len(c2p)
    assert L > 2 * BOOT_CHUNK and L % BOOT_CHUNK != 0
    assert P <= BOOT_LDS_BINS if case == "lds" else P > BOOT_LDS_BINS
    want = ref.counts(genes, None, SEED, rep)
    d = gpu_ctx.debug_boot_replicate(genes, None, SEED, rep, form=0)
    f = gpu_ctx.debug_boot_replicate(genes, None, SEED, rep, form=1)
    idx, npat = d["idx"], d["npat"]
    print("%s replicate %d: L %d, P %d, npat %d, max count %d" % (case, rep, L, P, npat, int(want.max())))
    assert np.array_equal(idx, ref.compact(want)) and npat == len(idx) <= P and np.array_equal(f["idx"], idx)
    w = d["weights"]
    assert np.array_equal(w[:npat], want[idx].astype(np.float64)) and w.sum() == L and not w[npat:].any()
    assert np.array_equal(f["weights"][:npat], want[idx]) and int(f["weights"].sum()) == L
    gnames, codes, _ = gpu_ctx.debug_gather(genes, None)
    assert np.array_equal(d["cells"][:, :npat], codes[:, idx]) and np.all(d["cells"][:, npat:] == 22)
    assert np.array_equal(f["cells"][:, :npat], MASK[codes[:, idx]])
    # the pair counts over the materialised text
    names, rows = ref.materialise(genes, None, SEED, rep)
    enc = _encode_text(rows)
    ok = enc < 20
    okp = ok[:, None, :] & ok[None, :, :]
    cmp_, diff = okp.sum(axis=2), (okp & (enc[:, None, :] != enc[None, :, :])).sum(axis=2)
    np.fill_diagonal(cmp_, 0); np.fill_diagonal(diff, 0)
    assert names == d["names"] and np.array_equal(d["cmp"], cmp_) and np.array_equal(d["diff"], diff)


_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from pepr_amd import engine
import test_gpu_boot as t
ctx = engine.Context(0)
out = {}
for si, sel in enumerate(t.SELS):
    for rep in t.KERNEL_REPS:
        for form in (0, 1):
            d = ctx.debug_boot_replicate(t.GENES, sel, t.SEED, rep, form=form)
            for k in ("idx", "cells", "weights", "cmp", "diff"):
                out["%d_%d_%d_%s" % (si, rep, form, k)] = d[k]
for case in sorted(t.WIDE):
    for rep in t.WIDE_REPS:
        d = ctx.debug_boot_replicate(t.WIDE[case], None, t.SEED, rep, form=0)
        for k in ("idx", "cells", "weights", "cmp", "diff"):
            out["%s_%d_%s" % (case, rep, k)] = d[k]
np.savez(sys.argv[2], **out)
ctx.close()
"""


def test_global_histogram_gives_the_same_bytes(gpu_ctx, tmp_path):
    """PML_BOOT_GLOBAL_HIST=1 (a child process: the switch is read per call, the child keeps this process's environment clean)
    forces k_boot_count's global-atomics form; integer adds commute, so every byte downstream is the same"""
    script, out = tmp_path / "child.py", tmp_path / "global.npz"
    script.write_text(_CHILD)
    env = dict(os.environ, PML_BOOT_GLOBAL_HIST="1")
    p = subprocess.run([sys.executable, str(script), ROOT, str(out)], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    got = np.load(str(out))
    assert "PML_BOOT_GLOBAL_HIST" not in os.environ
    for si, sel in enumerate(SELS):
        for rep in KERNEL_REPS:
            for form in (0, 1):
                d = gpu_ctx.debug_boot_replicate(GENES, sel, SEED, rep, form=form)
                for k in ("idx", "cells", "weights", "cmp", "diff"):
                    a = got["%d_%d_%d_%s" % (si, rep, form, k)]
                    assert a.dtype == d[k].dtype and a.tobytes() == d[k].tobytes(), (sel, rep, form, k)
    # three workgroups per replicate: the forced global form against the LDS form's per-bin flush ("lds"), and against itself
    # where the call had switched to it anyway ("auto")
    for case in sorted(WIDE):
        for rep in WIDE_REPS:
            d = gpu_ctx.debug_boot_replicate(WIDE[case], None, SEED, rep, form=0)
            for k in ("idx", "cells", "weights", "cmp", "diff"):
                a = got["%s_%d_%s" % (case, rep, k)]
                assert a.dtype == d[k].dtype and a.tobytes() == d[k].tobytes(), (case, rep, k)


# ---- 2. the parsimony bootstrap against the oracle (exact) ----
@pytest.fixture(scope="module")
def pars20(gpu_ctx):
    return gpu_ctx.bootstrap2(GENES, reps=REPS, seed=SEED, method=PARSIMONY, parsimony_radius=20)


@pytest.mark.parametrize("radius", [20, 0])
def test_parsimony_bootstrap_vs_oracle(gpu_ctx, oracle_lib, materialised, pars20, radius):
    po = oracle_lib
    r = pars20 if radius == 20 else gpu_ctx.bootstrap2(GENES, reps=REPS, seed=SEED, method=PARSIMONY, parsimony_radius=0)
    assert len(r["replicates"]) == REPS and len(r["mp_lengths"]) == 1 + REPS and r["replicate_lnl"] == []
    for i in range(REPS):
        names, rows = materialised(None, i)
        t, olen, _ = po.parsimony_tree(po.Alignment(names, rows), REP_SEEDS[i], radius)
        got = r["replicates"][i]
        print("replicate %d: length %d (oracle %d)" % (i, r["mp_lengths"][1 + i], olen))
        assert ":" not in got and _leaves(got) == sorted(names)
        assert r["mp_lengths"][1 + i] == olen == util.fitch_length(names, rows, got)
        assert engine.rf_distance(got, t.newick()) == 0
    # the best tree: the oracle's on the concatenated text
    names, rows = engine.concatenate(GENES)
    t, olen, _ = po.parsimony_tree(po.Alignment(names, rows), FULL_SEED, radius)
    assert ":" not in r["newick"] and engine.rf_distance(_strip(r["newick"]), t.newick()) == 0 and r["mp_lengths"][0] == olen
    assert r["lnl"] == 0 and r["alpha"] == 0 and r["tree_length"] == 0
    assert r["nsites"] == len(rows[0]) and r["npatterns"] == ref.col2pat(GENES)[1]
    # the labels: a recount of the returned replicate trees
    labels = sorted(int(x) for x in re.findall(r"\)(\d+)", r["newick"]))
    assert len(labels) == len(names) - 3 and labels == _labels_recount(r["newick"], r["replicates"], REPS)


def test_parsimony_bl(gpu_ctx, pars20):
    r = gpu_ctx.bootstrap2(GENES, reps=REPS, seed=SEED, method=PARSIMONY_BL, parsimony_radius=20)
    assert ":" in r["newick"] and r["lnl"] < 0 and r["alpha"] > 0 and r["tree_length"] > 0
    assert engine.rf_distance(re.sub(r"\)\d+:", "):", r["newick"]), _strip(pars20["newick"])) == 0
    assert r["replicates"] == pars20["replicates"] and all(":" not in t for t in r["replicates"])       # topology only: nothing reads their lengths
    assert r["mp_lengths"] == pars20["mp_lengths"]
    assert sorted(int(x) for x in re.findall(r"\)(\d+):", r["newick"])) == sorted(int(x) for x in re.findall(r"\)(\d+)", pars20["newick"]))


# ---- 3. the ML bootstrap against the oracle ----
ML_REPS = 3
_, _, ML_GENES = _sliced_genes(12, 4, 120, 31)


@pytest.fixture(scope="module")
def ml_run(gpu_ctx):
    return gpu_ctx.bootstrap2(ML_GENES, reps=ML_REPS, seed=SEED, method=ML, spr_radius=5)


def test_ml_bootstrap_vs_oracle(oracle_lib, materialised, ml_run):
    """the project's rule for a replicate on concatenated text (test_jackknife_vs_oracle_on_concatenated_text): against the oracle's
    search from its NJ tree, RF 0 (branches the tree itself holds at zero length aside) and |dlnL| < 1e-3"""
    po = oracle_lib
    r = ml_run
    m = po.Model(0)
    assert len(r["replicates"]) == ML_REPS == len(r["replicate_lnl"]) and r["mp_lengths"] == [-1] * (1 + ML_REPS)
    for i in range(ML_REPS):
        names, rows = materialised(None, i, ML_GENES)
        a = po.Alignment(names, rows); e = po.Engine(a, m, 4, 1.0)
        lnl_o, t_o = e.search(None, 0, 1e-3)
        print("replicate %d: lnL %.6f (oracle %.6f)" % (i, r["replicate_lnl"][i], lnl_o))
        assert util.rf_collapsed(r["replicates"][i], t_o.newick()) == 0
        assert abs(r["replicate_lnl"][i] - lnl_o) < 1e-3
        assert abs(e.lnl(po.Tree(r["replicates"][i], a)) - lnl_o) < 1e-3          # the tree as returned, under the oracle's alpha
    names, rows = engine.concatenate(ML_GENES)
    a = po.Alignment(names, rows); e = po.Engine(a, m, 4, 1.0)
    lnl_o, t_o = e.search(None, 5, 1e-3)
    assert abs(r["lnl"] - lnl_o) < 1e-3 and abs(r["alpha"] - e.alpha) < 1e-3 * e.alpha
    assert util.rf_collapsed(re.sub(r"\)\d+:", "):", r["newick"]), t_o.newick()) == 0
    labels = sorted(int(x) for x in re.findall(r"\)(\d+):", r["newick"]))
    assert len(labels) == len(names) - 3 and labels == _labels_recount(re.sub(r":[0-9.eE+-]+", "", r["newick"]), r["replicates"], ML_REPS)


def test_ml_bootstrap_empirical_frequencies(gpu_ctx, oracle_lib, materialised):
    """a per-gene code: every replicate gets its own model, its frequencies counted on the device from the replicate's matrix and
    weights -- the oracle counts them from the materialised text"""
    po = oracle_lib
    r = gpu_ctx.bootstrap2(ML_GENES, reps=2, seed=SEED, method=ML, pi_mode=engine.PI_EMPIRICAL)
    for i in range(2):
        names, rows = materialised(None, i, ML_GENES)
        a = po.Alignment(names, rows); e = po.Engine(a, po.Model(pi=po.empirical_freqs(a)), 4, 1.0)
        lnl_o, t_o = e.search(None, 0, 1e-3)
        print("replicate %d under empirical frequencies: lnL %.6f (oracle %.6f)" % (i, r["replicate_lnl"][i], lnl_o))
        assert abs(r["replicate_lnl"][i] - lnl_o) < 1e-3


def test_ml_bootstrap_gtr(gpu_ctx):
    _, _, genes = _sliced_genes(6, 4, 120, 29)                       # the case of test_gtr_replicates
    g = gpu_ctx.bootstrap2(genes, reps=2, seed=SEED, method=ML, epsilon=EPS_GTR, pi_mode=engine.PI_GTR)
    f = gpu_ctx.bootstrap2(genes, reps=2, seed=SEED, method=ML, epsilon=EPS_GTR, pi_mode=engine.PI_EMPIRICAL)
    assert len(g["replicates"]) == 2 and np.isfinite(g["lnl"])
    for i in range(2):
        print("replicate %d: GTR lnL %.6f, WAGF %.6f" % (i, g["replicate_lnl"][i], f["replicate_lnl"][i]))
        assert g["replicate_lnl"][i] >= f["replicate_lnl"][i]


def test_replicate_model(gpu_ctx, ml_run):
    """replicate_model: another code for the replicates than for the best tree"""
    r = gpu_ctx.bootstrap2(ML_GENES, reps=ML_REPS, seed=SEED, method=ML, spr_radius=5, replicate_pi_mode=engine.PI_EMPIRICAL)
    f = gpu_ctx.bootstrap2(ML_GENES, reps=ML_REPS, seed=SEED, method=ML, spr_radius=5, pi_mode=engine.PI_EMPIRICAL)
    assert _strip(r["newick"]) == _strip(ml_run["newick"])         # the best tree is built under `model`
    assert r["lnl"] == ml_run["lnl"] and r["replicates"] == f["replicates"] and r["replicate_lnl"] == f["replicate_lnl"]


# ---- 4. determinism and structure ----
def test_determinism(gpu_ctx, pars20, ml_run):
    again = gpu_ctx.bootstrap2(GENES, reps=REPS, seed=SEED, method=PARSIMONY, parsimony_radius=20)
    assert again == pars20
    again = gpu_ctx.bootstrap2(ML_GENES, reps=ML_REPS, seed=SEED, method=ML, spr_radius=5)
    assert again == ml_run
    a, b = gpu_ctx.debug_boot_replicate(GENES, None, SEED, 2), gpu_ctx.debug_boot_replicate(GENES, None, SEED + 1, 2)
    assert not np.array_equal(a["idx"], b["idx"])
    c = gpu_ctx.debug_boot_replicate(GENES, None, SEED, 2)
    assert all(a[k].tobytes() == c[k].tobytes() for k in ("idx", "cells", "weights", "cmp", "diff"))


def test_reps_zero(gpu_ctx, pars20, ml_run):
    r = gpu_ctx.bootstrap2(GENES, reps=0, seed=SEED, method=PARSIMONY, parsimony_radius=20)
    assert r["replicates"] == [] and r["newick"] == _strip(pars20["newick"]) and not re.search(r"\)\d", r["newick"])
    one = gpu_ctx.parsimony([engine.concatenate(GENES)], seed=FULL_SEED, spr_radius=20)[0]
    assert engine.rf_distance(r["newick"], one["newick"]) == 0 and r["mp_lengths"] == [one["length"]]
    r = gpu_ctx.bootstrap2(ML_GENES, reps=0, seed=SEED, method=ML, spr_radius=5)
    assert r["replicates"] == [] and not re.search(r"\)\d+:", r["newick"]) and r["lnl"] == ml_run["lnl"]
    one = gpu_ctx.search([engine.concatenate(ML_GENES)], None, nni=True, spr_radius=5)[0]
    assert engine.rf_distance(r["newick"], one["newick"]) == 0 and abs(r["lnl"] - one["lnl"]) < 1e-3


def test_sub_batching(gpu_ctx, pars20, ml_run, monkeypatch):
    monkeypatch.setenv("PML_HBM_BUDGET_MB", "1")                  # every replicate exceeds it: one sub-batch each
    before = gpu_ctx.boot_stats()["launches"]
    r = gpu_ctx.bootstrap2(GENES, reps=REPS, seed=SEED, method=PARSIMONY, parsimony_radius=20)
    after = gpu_ctx.boot_stats()["launches"]
    assert {k: after[k] - before[k] for k in after} == {"count": REPS, "index": REPS, "gather": REPS, "pairs": 0}
    assert r == pars20
    r = gpu_ctx.bootstrap2(ML_GENES, reps=ML_REPS, seed=SEED, method=ML, spr_radius=5)
    last = gpu_ctx.boot_stats()["launches"]
    assert {k: last[k] - after[k] for k in last} == {"count": ML_REPS, "index": ML_REPS, "gather": ML_REPS, "pairs": ML_REPS}
    assert r["newick"] == ml_run["newick"] and r["replicates"] == ml_run["replicates"]
    monkeypatch.delenv("PML_HBM_BUDGET_MB")
    before = gpu_ctx.boot_stats()["launches"]
    gpu_ctx.bootstrap2(ML_GENES, reps=ML_REPS, seed=SEED, method=ML, spr_radius=5)
    after = gpu_ctx.boot_stats()["launches"]
    assert {k: after[k] - before[k] for k in after} == {"count": 1, "index": 1, "gather": 1, "pairs": 1}      # one sub-batch, one launch each


def test_one_gene(gpu_ctx, oracle_lib, materialised):
    po = oracle_lib
    gene = GENES[1]
    r = gpu_ctx.bootstrap2([gene], reps=2, seed=SEED, method=PARSIMONY)
    for i in range(2):
        names, rows = materialised([1], i)
        assert names == sorted(gene[0])
        t, olen, _ = po.parsimony_tree(po.Alignment(names, rows), REP_SEEDS[i], 20)
        assert r["mp_lengths"][1 + i] == olen and engine.rf_distance(r["replicates"][i], t.newick()) == 0


def test_refusals(gpu_ctx):
    before = gpu_ctx.boot_stats()
    for kw, word in ((dict(reps=-1), "reps"), (dict(method=7), "method"), (dict(method=-1), "method"), (dict(method=PARSIMONY, parsimony_radius=-1), "radius"),
                     (dict(pi_mode=9), "pi_mode")):
        with pytest.raises(engine.PmlError) as e:
            gpu_ctx.bootstrap2(GENES, **{"reps": 2, **kw})
        assert e.value.code == engine.EINVAL and word in str(e.value), kw
    two = (["a", "a", "b"], ["ARND", "ARNE", "ARNQ"])               # a union of two taxa
    for method in (ML, PARSIMONY):
        with pytest.raises(engine.PmlError) as e:
            gpu_ctx.bootstrap2([two], reps=2, method=method)
        assert e.value.code == engine.EINVAL and "fewer than 3 taxa" in str(e.value)
    # L >= 2^31: two genes that claim 2^30 columns each; refused from the column counts alone, before a row is read
    keep = []
    alns = (_lib.Alignment * 2)(*[engine._aln_struct(g[0], g[1], keep) for g in GENES[:2]])
    alns[0].nsites = alns[1].nsites = 1 << 30
    m, o = engine._model(), _lib.BootstrapOpts2(2, ML, SEED, 5, 20, 0.0, None)
    import ctypes as C
    res = _lib.Result()
    rc = gpu_ctx.L.pml_bootstrap2(gpu_ctx.ptr, 2, alns, C.byref(m), C.byref(o), C.byref(res), None, None)
    assert rc == engine.EINVAL and "2^31" in gpu_ctx.L.pml_last_error(gpu_ctx.ptr).decode()
    assert gpu_ctx.boot_stats() == before                           # refused before anything ran


def test_mirror_and_command(gpu_ctx, tmp_path):
    from pepr_amd import tree_builder as tb
    got = tb.buildConcatenatedTree(GENES, 3, tb.PARSIMONY, "PROTGAMMAWAG", ctx=gpu_ctx, seed=2, details=True)
    want = gpu_ctx.bootstrap2(GENES, reps=3, seed=2, method=PARSIMONY, spr_radius=5, parsimony_radius=20)
    assert got == want and tb.buildConcatenatedTree(GENES, 3, tb.PARSIMONY, "PROTGAMMAWAG", ctx=gpu_ctx, seed=2) == want["newick"]
    d = tmp_path / "aln"
    d.mkdir()
    for i, (nm, rw) in enumerate(GENES):
        (d / ("g%d.faa" % i)).write_text("".join(">%s\n%s\n" % (n, r) for n, r in zip(nm, rw)))
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "pepr_tree_step.py"), "-run_name", "r", "-alignment_dir", str(d), "-concatenated",
                        "-support_reps", "3", "-seed", "2", "--full-tree-method", "parsimony"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    assert "parsimony length" in p.stdout
    assert (tmp_path / "r.nwk").read_text().strip() == want["newick"] and (tmp_path / "r.sup").read_text().split() == want["replicates"]
