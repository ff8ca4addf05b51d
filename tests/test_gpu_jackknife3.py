"""pml_jackknife3: parsimony support trees and parsimony full trees from the genes resident in HBM.  k_fitch_tips writes the
Fitch tip vectors of every replicate straight from the genes' code matrices; everything downstream is integer work, so trees
and Fitch lengths equal the C oracle's on the concatenated text exactly."""
import collections
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import util
from pepr_amd import engine, synth, tree_builder as tb
from test_gpu_jackknife import _encode_text

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ML, PARSIMONY, PARSIMONY_BL = engine.TREE_ML, engine.TREE_PARSIMONY, engine.TREE_PARSIMONY_BL
MASK = np.array([1 << c for c in range(20)] + [(1 << 2) | (1 << 3), (1 << 5) | (1 << 6), 0xFFFFF], dtype=np.uint32)   # code -> state set
REPS, SEED = 5, 3


def _genes():
    """segments below 32 patterns and above 256, dst_off values that are multiples of nothing, genes that lack taxa of the
    union, B / Z / X / - / ? residues"""
    genes = []
    keep = {0: 12, 2: 9, 4: 7, 1: 12, 3: 12, 5: 11}
    for i, m in enumerate([37, 300, 257, 64, 5, 130]):
        names, rows, _ = synth.simulate_alignment(12, m, 4000 + i, missing_frac=0.1 if i % 2 else 0.0)
        names, rows = (names[-keep[i]:], rows[-keep[i]:]) if i % 2 else (names[:keep[i]], rows[:keep[i]])
        rows = [r[:3] + "BZX-?"[j % 5] + r[4:] for j, r in enumerate(rows)]
        genes.append((names, rows))
    return genes


GENES = _genes()
DRAW = engine.jackknife_draw(len(GENES), REPS, 0, SEED)
FULL_SEED, REP_SEEDS = engine.jackknife_parsimony_seeds(SEED, REPS)


def _strip(nw):
    return re.sub(r"\)\d+", ")", nw)


def _leaves(nw):
    return sorted(re.findall(r"[(,]([^(),:;]+)", nw))


@pytest.fixture(scope="module")
def oracle_trees(oracle_lib):
    """the oracle's parsimony trees of the concatenated text: {(selection, seed, radius): (newick, length)}, built once"""
    po = oracle_lib
    cache = {}

    def get(sel, seed, radius):
        key = (tuple(sel), seed, radius)
        if key not in cache:
            names, rows = engine.concatenate(GENES, list(sel))
            t, length, _ = po.parsimony_tree(po.Alignment(names, rows), seed, radius)
            cache[key] = (t.newick(), length, names, rows)
        return cache[key]
    return get


@pytest.fixture(scope="module")
def run20(gpu_ctx):
    """the reference run of most tests: parsimony throughout, radius 20, rule 0"""
    return gpu_ctx.jackknife3(GENES, reps=REPS, seed=SEED, full_method=PARSIMONY, support_method=PARSIMONY, parsimony_radius=20)


# ---- 1. the tips kernel alone ----
@pytest.mark.parametrize("sel", [None, [4], [2, 4], [1, 3, 5]])
def test_fitch_tips_kernel(gpu_ctx, sel):
    before = gpu_ctx.fitch_stats()
    names, masks, w, npat = gpu_ctx.debug_fitch_tips(GENES, sel)
    after = gpu_ctx.fitch_stats()
    assert after["tips_launches"] == before["tips_launches"] + 1 and after["fitch_launches"] == before["fitch_launches"]
    gnames, codes, gw = gpu_ctx.debug_gather(GENES, sel)
    assert names == gnames and codes.shape[1] == npat and masks.shape == (len(names), (npat + 31) // 32 * 32)
    want = np.full(masks.shape, 0xFFFFF, dtype=np.uint32)              # padding patterns: every state, weight 0
    want[:, :npat] = MASK[codes]
    assert np.array_equal(masks, want)
    assert np.array_equal(w[:npat], gw.astype(np.int64)) and not w[npat:].any() and (w[:npat] > 0).all()
    # independent of any device code: {column of state sets -> number of sites} from the concatenated text
    tnames, rows = engine.concatenate(GENES, sel)
    assert tnames == names
    text = collections.Counter(map(tuple, MASK[_encode_text(rows)].T.tolist()))
    dev = collections.Counter()
    for p in range(npat):
        dev[tuple(masks[:, p].tolist())] += int(w[p])
    assert dev == text
    if sel == [4]:
        assert npat < 32
    if sel is None:
        assert npat > 256 and any(len(g[0]) < len(names) for g in GENES)     # a second pattern block; absent-taxon rows


# ---- 2. support trees against the oracle ----
@pytest.mark.parametrize("radius", [20, 0])
def test_support_trees_vs_oracle(gpu_ctx, oracle_trees, run20, radius):
    r = run20 if radius == 20 else gpu_ctx.jackknife3(GENES, reps=REPS, seed=SEED, full_method=PARSIMONY, support_method=PARSIMONY, parsimony_radius=0)
    assert len(r["support_trees"]) == REPS and len(r["mp_lengths"]) == 1 + REPS
    for i, sel in enumerate(DRAW):
        onw, olen, names, rows = oracle_trees(sel, REP_SEEDS[i], radius)
        got = r["support_trees"][i]
        print("replicate %d genes %s: length %d (oracle %d)" % (i, sel, r["mp_lengths"][1 + i], olen))
        assert ":" not in got and _leaves(got) == sorted(names)
        assert r["mp_lengths"][1 + i] == olen == util.fitch_length(names, rows, got)
        assert engine.rf_distance(got, onw) == 0
    if radius == 20:          # the genes were chosen so that SPR moves happen and the seed matters
        zero = [oracle_trees(sel, REP_SEEDS[i], 0)[1] for i, sel in enumerate(DRAW)]
        assert any(z > l for z, l in zip(zero, r["mp_lengths"][1:]))
        assert all(any(len(GENES[g][0]) < len(_leaves(t)) for g in sel) for sel, t in zip(DRAW, r["support_trees"]))   # absent-taxon rows in every replicate


# ---- 3. counts ----
@pytest.mark.parametrize("rule", [0, 1, 2])
def test_support_counts(gpu_ctx, run20, rule):
    r = run20 if rule == 0 else gpu_ctx.jackknife3(GENES, reps=REPS, seed=SEED, full_method=PARSIMONY, support_method=PARSIMONY,
                                                   parsimony_radius=20, support_rule=rule)
    assert r["support_trees"] == run20["support_trees"]
    main = _strip(r["newick"])
    assert main == _strip(run20["newick"]) and re.search(r"\)\d+", r["newick"])
    if rule == 0:
        full_set = [t for t in r["support_trees"] if _leaves(t) == _leaves(main)]
        assert r["newick"] == engine.support_tree(main, full_set, digits=-1)
    else:
        assert r["newick"] == engine.support_tree_rule(main, r["support_trees"], rule, digits=-1)


# ---- 4. full tree, parsimony ----
def test_full_tree_parsimony(oracle_trees, run20):
    onw, olen, names, rows = oracle_trees(range(len(GENES)), FULL_SEED, 20)
    assert ":" not in run20["newick"]
    assert engine.rf_distance(_strip(run20["newick"]), onw) == 0 and run20["mp_lengths"][0] == olen
    assert run20["lnl"] == 0 and run20["alpha"] == 0 and run20["tree_length"] == 0
    assert run20["nsites"] == len(rows[0]) == sum(len(g[1][0]) for g in GENES) and 0 < run20["npatterns"] <= run20["nsites"]


# ---- 5. full tree, parsimony_bl ----
def test_full_tree_parsimony_bl(gpu_ctx, oracle_lib, run20):
    """the bounds of test_optimize_vs_oracle (north-star tolerance): |dlnL| < 1e-3, alpha to 1e-4 max(1, alpha)"""
    po = oracle_lib
    r = gpu_ctx.jackknife3(GENES, reps=0, seed=SEED, epsilon=1e-4, full_method=PARSIMONY_BL, support_method=PARSIMONY, parsimony_radius=20)
    assert ":" in r["newick"] and engine.rf_distance(r["newick"], _strip(run20["newick"])) == 0
    assert r["mp_lengths"] == [run20["mp_lengths"][0]]
    names, rows = engine.concatenate(GENES)
    aln = po.Alignment(names, rows)
    t, _, _ = po.parsimony_tree(aln, FULL_SEED, 20)
    e = po.Engine(aln, po.Model(0), 4, 1.0)
    lnl = e.optimize(t, True, 1e-4)
    print("parsimony_bl: lnL %.6f (oracle %.6f), alpha %.6f (oracle %.6f)" % (r["lnl"], lnl, r["alpha"], e.alpha))
    assert abs(r["lnl"] - lnl) < 1e-3
    assert abs(r["alpha"] - e.alpha) < 1e-4 * max(1.0, e.alpha)
    again = gpu_ctx.score([(names, rows)], [r["newick"]], alpha=r["alpha"])[0]["lnl"]
    assert abs(again - r["lnl"]) < 1e-6
    assert r["tree_length"] > 0 and r["nsites"] == len(rows[0])


# ---- 6. defaults ----
def test_both_methods_ml_is_jackknife2(gpu_ctx):
    kw = dict(reps=3, seed=SEED, spr_radius_full=5, support_rule=1)
    a = gpu_ctx.jackknife3(GENES, full_method=ML, support_method=ML, **kw)
    b = gpu_ctx.jackknife2(GENES, **kw)
    for k in ("newick", "support_trees", "lnl", "alpha", "tree_length", "npatterns", "nsites"):
        assert a[k] == b[k], k
    assert a["mp_lengths"] == [-1] * 4


# ---- 7. sharding ----
def test_sharding(gpu_ctx, run20):
    parts = [gpu_ctx.jackknife3(GENES, reps=REPS, seed=SEED, full_method=PARSIMONY, support_method=PARSIMONY, parsimony_radius=20, shard=(k, 2))
             for k in (0, 1)]
    # the full tree appears on rank 0 alone, counted over that rank's replicates; the caller gathers and decorates
    assert _strip(parts[0]["newick"]) == _strip(run20["newick"]) and parts[1]["newick"] is None
    trees = [None] * REPS
    trees[0::2], trees[1::2] = parts[0]["support_trees"], parts[1]["support_trees"]
    assert trees == run20["support_trees"]
    assert engine.support_tree_rule(_strip(parts[0]["newick"]), trees, 0, digits=-1) == run20["newick"]
    assert parts[0]["mp_lengths"] == [run20["mp_lengths"][0]] + [v if r % 2 == 0 else -1 for r, v in enumerate(run20["mp_lengths"][1:])]
    assert parts[1]["mp_lengths"] == [-1] + [v if r % 2 == 1 else -1 for r, v in enumerate(run20["mp_lengths"][1:])]


# ---- 8. sub-batching ----
def test_sub_batching(gpu_ctx, run20, monkeypatch):
    monkeypatch.setenv("PML_HBM_BUDGET_MB", "1")              # every replicate's pool exceeds it: one sub-batch each
    before = gpu_ctx.fitch_stats()
    r = gpu_ctx.jackknife3(GENES, reps=REPS, seed=SEED, full_method=PARSIMONY, support_method=PARSIMONY, parsimony_radius=20)
    after = gpu_ctx.fitch_stats()
    assert after["tips_launches"] - before["tips_launches"] == 1 + REPS
    for k in ("newick", "support_trees", "mp_lengths"):
        assert r[k] == run20[k], k


# ---- 9. launch counters and refusals ----
def test_launch_counters_and_refusals(gpu_ctx):
    before = gpu_ctx.fitch_stats()
    gpu_ctx.jackknife3(GENES, reps=REPS, seed=SEED, support_method=PARSIMONY, shard=(1, 2))       # no full tree on rank 1: one sub-batch
    mid = gpu_ctx.fitch_stats()
    assert mid["tips_launches"] == before["tips_launches"] + 1 and mid["fitch_launches"] > before["fitch_launches"]
    gpu_ctx.parsimony([GENES[1]], seed=2)
    after = gpu_ctx.fitch_stats()
    assert after["tips_launches"] == mid["tips_launches"] and after["fitch_launches"] > mid["fitch_launches"]
    with pytest.raises(engine.PmlError) as e:
        gpu_ctx.jackknife3(GENES, reps=2, support_method=PARSIMONY_BL)
    assert e.value.code == engine.EINVAL and "lengths" in str(e.value)
    for kw in (dict(support_method=7), dict(full_method=7), dict(full_method=-1), dict(support_method=PARSIMONY, parsimony_radius=-1)):
        with pytest.raises(engine.PmlError) as e:
            gpu_ctx.jackknife3(GENES, reps=2, **kw)
        assert e.value.code == engine.EINVAL
    assert gpu_ctx.fitch_stats() == after                                 # refused before anything ran
    # a replicate whose taxon union has two taxa (a gene that names a taxon twice)
    two = (["a", "a", "b"], ["ARND", "ARNE", "ARNQ"])
    seed = next(s for s in range(1, 100) if [1] in engine.jackknife_draw(2, 4, 1, s)[1:])      # drawn, and not as replicate 0
    draw = engine.jackknife_draw(2, 4, 1, seed)
    with pytest.raises(engine.PmlError) as e:
        gpu_ctx.jackknife3([GENES[0], two], reps=4, subset_size=1, seed=seed, full_method=PARSIMONY, support_method=PARSIMONY)
    assert e.value.code == -2 and "replicate %d: parsimony needs at least 3 taxa" % draw.index([1]) in str(e.value)


# ---- 10. the pipeline mirror and the command ----
def test_mirror_and_command(gpu_ctx, tmp_path):
    got = tb.buildConcatenatedTreeWithGeneWiseJackKnifeSupport(GENES, reps=3, supportTreeMethod=tb.PARSIMONY, ctx=gpu_ctx, seed=2)
    want = gpu_ctx.jackknife3(GENES, reps=3, seed=2, spr_radius_full=5, support_rule=1, support_method=PARSIMONY, parsimony_radius=20)
    assert got == want and ":" in got["newick"] and all(":" not in t for t in got["support_trees"])
    got = tb.buildConcatenatedTreeWithGeneWiseJackKnifeSupport(GENES, reps=2, fullTreeMethod=tb.PARSIMONY_BL, ctx=gpu_ctx, seed=2)
    want = gpu_ctx.jackknife3(GENES, reps=2, seed=2, spr_radius_full=5, support_pi_mode=engine.PI_WAG_FULL, support_rule=1,
                              full_method=PARSIMONY_BL, parsimony_radius=20)
    assert got == want and got["lnl"] < 0 and all(":" in t for t in got["support_trees"])
    d = tmp_path / "aln"
    d.mkdir()
    for i, (nm, rw) in enumerate(GENES):
        (d / ("g%d.faa" % i)).write_text("".join(">%s\n%s\n" % (n, r) for n, r in zip(nm, rw)))
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "pepr_tree_step.py"), "-run_name", "r", "-alignment_dir", str(d),
                        "-support_reps", "3", "-seed", "2", "--support-tree-method", "parsimony", "--full-tree-method", "parsimony"],
                       cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    assert "parsimony length" in p.stdout and "lnL" not in p.stdout
    step = gpu_ctx.jackknife3(GENES, reps=3, seed=2, support_rule=1, full_method=PARSIMONY, support_method=PARSIMONY)
    assert (tmp_path / "r.nwk").read_text().strip() == step["newick"] and ":" not in step["newick"]
    assert (tmp_path / "r.sup").read_text().split() == step["support_trees"] and ":" not in "".join(step["support_trees"])
