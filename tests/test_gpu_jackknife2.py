"""pml_jackknife2: the gene-wise jackknife under the model the pipeline chose (per-replicate "F" / GTR models, their
frequencies counted on the device by k_codehist; another model for the support trees) and with the decorator's support
counts (TreeSupportDecorator.addSupportValues on the returned strings, tests/decorator_ref.py)."""
import os
import socket
import sys

import numpy as np
import pytest

import decorator_ref as dr
from pepr_amd import engine, synth
from test_gpu_jackknife import _encode_text, _sliced_genes
from test_gpu_models import oracle_model, random_matrix, simulate
from util import rf_collapsed

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. k_codehist through pml_debug_replicate_freqs ----

def _distinct_columns(ntax, ncol, seed):
    """an alignment whose columns are all different (so npat = ncol exactly)"""
    rng = np.random.default_rng(seed)
    cols = set()
    while len(cols) < ncol:
        cols.add("".join(synth.AA[i] for i in rng.integers(0, 20, ntax)))
    cols = sorted(cols)
    return ["".join(c[t] for c in cols) for t in range(ntax)]


def _codehist_cases():
    cases = {}
    # genes lacking taxa of the union (gap rows), B / Z / X / - residues, npat no multiple of 32
    _, _, genes = _sliced_genes(9, 7, 64, 31)
    cases["sliced_all"] = (genes, None)
    cases["sliced_two_genes"] = (genes, [1, 4])                    # each lacks another taxon: gap rows, the union is still all 9
    cases["sliced_one_gene"] = (genes, [3])
    cases["sliced_8_taxa_beside_9"] = (genes, [1])                 # gene 1 has 8 taxa: two replicates of different ntax in one launch
    # a one-pattern gene and duplicate columns (weights > 1)
    names = ["x%d" % i for i in range(5)]
    one = (names, ["AAAAA", "CCCCC", "DDDDD", "AAAAA", "-----"])
    dup = (names[:4], ["ARARARNDND", "CCCCCCQEQE", "GGGGGGHIHI", "LKLKLKMFMF"])
    cases["one_pattern_gene_alone"] = ([one, dup], [0])
    cases["one_pattern_and_duplicates"] = ([one, dup], None)
    # all 23 codes present
    every = synth.AA + "BZX"
    cases["all_23_codes"] = ([(names, [every, every[::-1], every[5:] + every[:5], "-" * 23, "?" * 20 + "bzx"]), dup], None)
    # amino acids that never occur: the 0.001 floor
    few = (names, ["AAAACCCCAA", "ACACACACAC", "CCCCAAAADD", "ADADADADAD", "BBZZXX--AA"])
    cases["floor"] = ([few, (names[:3], ["ACD", "CDA", "DAC"])], None)
    # workgroup boundary: 257 patterns; 600 = 300 + 300 over two genes, the second lacking a taxon of the first -- and both
    # lacking s0, so the selection has 8 taxa and three workgroups of patterns beside the 9-taxon replicate of all genes
    n9 = ["s%d" % i for i in range(9)]
    cases["npat_257"] = ([(n9, _distinct_columns(9, 257, 1)), (n9[:4], _distinct_columns(4, 40, 2))], [0])
    cases["npat_600_8_taxa_beside_9"] = ([(n9[1:], _distinct_columns(8, 300, 3)), (n9[2:], _distinct_columns(7, 300, 4)), (n9[:3], ["AC", "CA", "AA"])], [0, 1])
    # the largest shape the 1e-12 bound was worked out for: 40 x 5000 characters
    nm, rows, _ = synth.simulate_alignment(40, 5000, 77, alpha=0.8, missing_frac=0.1)
    cases["40x5000"] = ([(nm, [r[:2500] for r in rows]), (nm[:37], [r[2500:] for r in rows[:37]])], None)
    return cases


CODEHIST = _codehist_cases()


@pytest.mark.parametrize("name", list(CODEHIST))
def test_codehist_counts_and_frequencies(gpu_ctx, oracle_lib, name):
    """counts: exactly numpy's count over the pml_concatenate text.  pi: the oracle's empirical_freqs of that text within
    1e-12 -- the two differ in summation order only (histogram restatement against the oracle on the CPU: 3.6e-16 at 9 x 260,
    2.3e-14 at 40 x 5000 characters, the largest shape here)."""
    po = oracle_lib
    genes, sel = CODEHIST[name]
    before = gpu_ctx.kernel_stats()["codehist"]
    counts, pi = gpu_ctx.debug_replicate_freqs(genes, sel)
    after = gpu_ctx.kernel_stats()["codehist"]
    assert after["launches"] == before["launches"] + 1           # one launch, whether one replicate or two
    nm, rows = engine.concatenate(genes, sel)
    want = np.bincount(_encode_text(rows).ravel(), minlength=23)
    assert counts.tolist() == want.tolist()
    ref = po.empirical_freqs(po.Alignment(nm, rows))
    print("%s: %d x %d characters, max |pi - oracle| = %.3g" % (name, len(rows), len(rows[0]), np.abs(pi - ref).max()))
    assert np.abs(pi - ref).max() < 1e-12
    if name == "all_23_codes":
        assert np.all(want > 0)
    if name == "floor":
        assert np.sum(want[:20] == 0) >= 10 and np.sum(np.abs(pi - 0.001) < 1e-15) >= 10
    if name.startswith("npat_"):
        npat = sum(len({"".join(r[c] for r in genes[g][1]) for c in range(len(genes[g][1][0]))}) for g in sel)
        assert npat == int(name.split("_")[1])
    if name.endswith("_8_taxa_beside_9"):                          # the hook launches the selection beside the replicate of all genes
        assert len(nm) == 8 and len(engine.concatenate(genes)[0]) == 9


# ---- 2. defaults drift nothing ----

def test_defaults_return_jackknifes_strings(gpu_ctx):
    _, _, genes = _sliced_genes(9, 6, 90, 23)
    a = gpu_ctx.jackknife(genes, reps=5, seed=4, spr_radius_full=5)
    b = gpu_ctx.jackknife2(genes, reps=5, seed=4, spr_radius_full=5)
    assert b["newick"] == a["newick"] and b["support_trees"] == a["support_trees"]
    assert b["lnl"] == a["lnl"] and b["alpha"] == a["alpha"]


# ---- 3. PML_PI_EMPIRICAL against the oracle on the concatenated text ----

def _check_against_oracle(po, r, genes, draws, model_of, spr_full=5):
    """the full tree and replicate 1 of result r against oracle searches on the concatenated text (the tolerances of
    test_jackknife_vs_oracle_on_concatenated_text); model_of(alignment) -> the oracle's model for that text"""
    nm, rows = engine.concatenate(genes)
    a = po.Alignment(nm, rows); e = po.Engine(a, model_of(a), 4, 1.0)
    lnl_o, t_o = e.search(None, spr_full, 1e-3)
    print("full tree: |dlnL| = %.3g, alpha %.6f vs %.6f" % (abs(r["lnl"] - lnl_o), r["alpha"], e.alpha))
    assert rf_collapsed(r["newick"], t_o.newick()) == 0
    assert abs(r["lnl"] - lnl_o) < 1e-3 and abs(r["alpha"] - e.alpha) < 1e-3 * e.alpha
    if draws is None:
        return
    nm, rows = engine.concatenate(genes, draws[1])
    a = po.Alignment(nm, rows); e = po.Engine(a, model_of(a), 4, 1.0)
    lnl_o, t_o = e.search(None, 0, 1e-3)
    sup = r["support_trees"][1]
    d = abs(e.lnl(po.Tree(sup, a)) - lnl_o)
    print("replicate 1: |dlnL| = %.3g" % d)
    assert rf_collapsed(sup, t_o.newick()) == 0
    assert d < 1e-3


def test_empirical_frequencies_vs_oracle_on_concatenated_text(gpu_ctx, oracle_lib):
    po = oracle_lib
    _, _, genes = _sliced_genes(8, 6, 110, 17)
    reps, seed = 3, 5
    r = gpu_ctx.jackknife2(genes, reps=reps, seed=seed, spr_radius_full=5, pi_mode=engine.PI_EMPIRICAL)
    assert len(r["support_trees"]) == reps
    draws = engine.jackknife_draw(len(genes), reps, 0, seed)
    _check_against_oracle(po, r, genes, draws, lambda a: po.Model(pi=po.empirical_freqs(a)))
    wag = gpu_ctx.jackknife(genes, reps=reps, seed=seed, spr_radius_full=5)
    assert abs(wag["lnl"] - r["lnl"]) > 1e-2                       # not WAG's own frequencies under another name


# ---- 4. two models ----

def test_registered_f_full_tree_and_wag_supports(gpu_ctx, oracle_lib):
    po = oracle_lib
    ex, pi = random_matrix(61)
    code = gpu_ctx.register_matrix("jk2", ex, pi)
    names, rows, _ = simulate(ex, pi, 8, 6 * 110, 4800)
    genes = []
    for g in range(6):
        nm, rw = list(names), [r[g * 110:(g + 1) * 110] for r in rows]
        if g % 3 == 1:
            nm, rw = nm[:g] + nm[g + 1:], rw[:g] + rw[g + 1:]
        genes.append((nm, rw))
    reps, seed = 3, 5
    r = gpu_ctx.jackknife2(genes, reps=reps, seed=seed, spr_radius_full=5, pi_mode=code + 1, support_pi_mode=engine.PI_RAXML_3DP)
    _check_against_oracle(po, r, genes, None, lambda a: oracle_model(po, ex, po.empirical_freqs(a)))
    wag = gpu_ctx.jackknife(genes, reps=reps, seed=seed, spr_radius_full=5)
    assert r["support_trees"] == wag["support_trees"]
    assert abs(r["lnl"] - wag["lnl"]) > 1e-2


# ---- 5. PML_PI_GTR ----

EPS_GTR = 0.01        # as tests/test_gpu_models.py: a rate sweep more costs seconds and pins nothing more
# |dlnL| of the full tree against the one-shot search on the concatenated text: 3.98e-06 observed on one MI355X (1.04e-05 at
# epsilon 1e-3); pinned at 8 x the observed value, and never above 1e-2
GTR_PIN = 3.2e-5


def test_gtr_replicates(gpu_ctx):
    """every replicate estimates its own exchangeabilities from the WAG start with the frequencies counted on the device"""
    _, _, genes = _sliced_genes(6, 4, 120, 29)
    r = gpu_ctx.jackknife2(genes, reps=2, seed=3, spr_radius_full=5, epsilon=EPS_GTR, pi_mode=engine.PI_GTR)
    assert len(r["support_trees"]) == 2 and np.isfinite(r["lnl"])
    f = gpu_ctx.jackknife2(genes, reps=2, seed=3, spr_radius_full=5, epsilon=EPS_GTR, pi_mode=engine.PI_EMPIRICAL)
    print("GTR full tree lnL %.6f, WAGF %.6f" % (r["lnl"], f["lnl"]))
    assert r["lnl"] >= f["lnl"] - 1e-3                             # GTR starts from WAG with the same frequencies and only accepts gains
    one = gpu_ctx.search([engine.concatenate(genes)], None, nni=True, spr_radius=5, epsilon=EPS_GTR, pi_mode=engine.PI_GTR)[0]
    print("GTR full tree against the one-shot search on the text: |dlnL| = %.3g" % abs(r["lnl"] - one["lnl"]))
    assert GTR_PIN <= 1e-2 and abs(r["lnl"] - one["lnl"]) < GTR_PIN
    assert engine.rf_distance(r["newick"], one["newick"]) == 0


# ---- 6. the rules end to end ----

RULE_REPS, RULE_SEED = 5, 5


def _rule_genes():
    """six genes of one 8-taxon alignment; t6 occurs in genes 0 and 1 only, t7 in gene 2 only"""
    names, rows, _ = synth.simulate_alignment(8, 600, 61, alpha=0.9)
    genes = []
    for g in range(6):
        keep = [i for i, n in enumerate(names) if not (n == "t6" and g not in (0, 1)) and not (n == "t7" and g != 2)]
        genes.append(([names[i] for i in keep], [rows[i][g * 100:(g + 1) * 100] for i in keep]))
    return genes


def _plain(newick):
    import re
    return re.sub(r"\)\d+:", "):", newick)


def _jk2_worker(rank, world, port, rule, q):
    sys.path.insert(0, ROOT)
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    from pepr_amd import distributed as pd
    pd.init_from_env(backend="gloo")
    ctx = engine.Context(0)                       # both ranks on the one GPU of the test box
    out = pd.jackknife(ctx, _rule_genes(), reps=RULE_REPS, seed=RULE_SEED, support_rule=rule, pi_mode=engine.PI_EMPIRICAL)
    if rank == 0:
        q.put({"newick": out["newick"], "support_trees": out["support_trees"]})
    dist.barrier()
    ctx.close()
    dist.destroy_process_group()


def test_rules_end_to_end(gpu_ctx):
    genes = _rule_genes()
    draws = engine.jackknife_draw(len(genes), RULE_REPS, 0, RULE_SEED)
    lacking = [d for d in draws if not ({0, 1} & set(d)) or 2 not in d]
    assert lacking and len(lacking) < RULE_REPS                    # the seed: replicates with and without every taxon
    got = {rule: gpu_ctx.jackknife2(genes, reps=RULE_REPS, seed=RULE_SEED, pi_mode=engine.PI_EMPIRICAL, support_rule=rule) for rule in (0, 1, 2)}
    sup = got[0]["support_trees"]
    plain = _plain(got[0]["newick"])
    for rule in (1, 2):
        assert got[rule]["support_trees"] == sup and _plain(got[rule]["newick"]) == plain
    assert any(t.count(",") < plain.count(",") for t in sup)      # a returned tree does lack a taxon
    assert dr.labelled_counts(got[1]["newick"]) == dr.decorator_counts(plain, sup)
    assert dr.labelled_counts(got[2]["newick"]) == dr.restricted_counts(plain, sup)
    for rule in (0, 1, 2):
        assert engine.support_tree_rule(plain, sup, rule, 6) == got[rule]["newick"]
    # rule 0 counts the replicates over the full taxon set only
    full = [t for t in sup if t.count(",") == plain.count(",")]
    assert got[0]["newick"] == engine.support_tree(plain, full, 6)
    # the sharded halves hold the same trees; their gather is the next test's
    halves = [gpu_ctx.jackknife2(genes, reps=RULE_REPS, seed=RULE_SEED, pi_mode=engine.PI_EMPIRICAL, support_rule=1, shard=(r, 2)) for r in range(2)]
    assert halves[0]["support_trees"] == sup[0::2] and halves[1]["support_trees"] == sup[1::2] and halves[1]["newick"] is None


def test_rules_sharded_over_two_ranks(gpu_ctx):
    """shard_world = 2 and the gather of distributed.jackknife (gloo, both ranks on GPU 0): the labels of the unsharded call"""
    import torch.multiprocessing as mp
    whole = gpu_ctx.jackknife2(_rule_genes(), reps=RULE_REPS, seed=RULE_SEED, pi_mode=engine.PI_EMPIRICAL, support_rule=1)
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_jk2_worker, args=(r, 2, port, 1, q)) for r in range(2)]
    for p in procs:
        p.start()
    out = q.get(timeout=300)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert out["support_trees"] == whole["support_trees"]
    assert out["newick"] == whole["newick"]


# ---- upper layers: the pipeline mirror and the command-line step ----

def test_mirror_and_tree_step_pass_the_matrix_through(gpu_ctx, tmp_path):
    import subprocess
    from pepr_amd import tree_builder as tb
    genes = _rule_genes()
    want = gpu_ctx.jackknife2(genes, reps=3, seed=1, spr_radius_full=5, pi_mode=engine.PI_EMPIRICAL,
                              support_pi_mode=engine.PI_WAG_FULL, support_rule=1)
    got = tb.buildConcatenatedTreeWithGeneWiseJackKnifeSupport([tb.SequenceAlignment(*g) for g in genes], reps=3,
                                                               mlMatrix="PROTGAMMAWAGF", ctx=gpu_ctx)
    assert got["newick"] == want["newick"] and got["support_trees"] == want["support_trees"]
    ml = tb.buildConcatenatedTreeWithGeneWiseJackKnifeSupport(genes, reps=3, supportTreeMethod=tb.ML, mlMatrix="PROTGAMMAWAGF", ctx=gpu_ctx)
    assert ml["newick"] == gpu_ctx.jackknife2(genes, reps=3, seed=1, pi_mode=engine.PI_EMPIRICAL, support_rule=1)["newick"]
    with pytest.raises(ValueError):
        tb.buildConcatenatedTreeWithGeneWiseJackKnifeSupport(genes, mlMatrix="PROTGAMMAJTT", ctx=gpu_ctx)
    d = tmp_path / "aln"
    d.mkdir()
    for i, (nm, rw) in enumerate(genes):
        (d / ("g%d.faa" % i)).write_text("".join(">%s\n%s\n" % (n, r) for n, r in zip(nm, rw)))
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "pepr_tree_step.py"), "-run_name", "r", "-alignment_dir", str(d),
                        "-support_reps", "3", "--matrix", "PROTGAMMAWAGF", "--support-matrix", "PROTGAMMAWAG", "--support-rule", "1"],
                       cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    step = gpu_ctx.jackknife2(genes, reps=3, seed=1, pi_mode=engine.PI_EMPIRICAL, support_pi_mode=engine.PI_RAXML_3DP, support_rule=1)
    assert (tmp_path / "r.nwk").read_text().strip() == step["newick"]
    assert (tmp_path / "r.sup").read_text().split() == step["support_trees"]
