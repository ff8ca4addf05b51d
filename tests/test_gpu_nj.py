"""The reference's `nj` tree-building method on the device: BLOSUM62 pair scores (k_pairscore, k_pairscore_sum) and the trees
TreeBuilder builds from them, against the line-by-line restatement tests/nj_ref.py.  Everything is integer sums and a fixed
sequence of double operations, so every comparison is exact: scores equal, tree texts equal in structure, every branch
length the same 8 bytes."""
import json
import os
import time

import numpy as np
import pytest

from pepr_amd import engine, tree_builder
import decorator_ref
import nj_ref

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
BLOSUM = json.load(open(os.path.join(GOLD, "blosum62_as_loaded.json")))["table"]
ALPHABET = "ARNDCQEGHILKMFPSTWYVBZX" + "arndcqeghilkmfpstwyvbzx" + "-?"        # all 24 codes, both cases


def _asymmetric_table():
    t = np.random.default_rng(62).integers(-128, 128, (24, 24))
    t[0, 0], t[23, 22], t[22, 23] = -128, 127, -77            # the whole int8 range, and a gap row / column that is not 0
    assert (t != t.T).any()
    return t


ASYM = _asymmetric_table()


def _rows(rng, ntax, nsites):
    return ["".join(rng.choice(list(ALPHABET), nsites)) for _ in range(ntax)]


def _same_tree(got, want):
    assert nj_ref.split_tree(got) == nj_ref.split_tree(want), (got, want)


# ---- 1. pml_pairwise_scores against the restatement ----
@pytest.mark.parametrize("nsites", [1, 63, 64, 65, 257, 1000])
@pytest.mark.parametrize("ntax", [2, 5, 17, 33, 65])
def test_pairwise_scores(gpu_ctx, ntax, nsites):
    rng = np.random.default_rng(1000 * ntax + nsites)
    names, rows = ["t%d" % i for i in range(ntax)], _rows(rng, ntax, nsites)
    for table, ref in ((None, BLOSUM), (ASYM, ASYM)):
        got = gpu_ctx.pairwise_scores((names, rows), table)
        want = nj_ref.pairwise_scores_np(rows, ref) - 1
        assert got.dtype == np.float64 and (got == want).all(), (ntax, nsites, np.argwhere(got != want)[:5])
    if ntax == 5 and nsites == 63:                         # the numpy restatement is the pure-Python one
        assert (np.array(nj_ref.pairwise_scores(rows, BLOSUM)) == nj_ref.pairwise_scores_np(rows, BLOSUM) - 1).all()


# ---- 2. chunk boundaries and the ends of the int8 range ----
@pytest.mark.parametrize("value", [127, -128])
def test_small_chunks_and_extreme_tables(gpu_ctx, value):
    rng = np.random.default_rng(7)
    names, rows = ["t%d" % i for i in range(7)], _rows(rng, 7, 1000)
    table = np.full((24, 24), value)
    want = nj_ref.pairwise_scores_np(rows, table)
    assert (want == 1000 * value).all()
    small = gpu_ctx.debug_pairscores((names, rows), table, chunk_sites=64)          # 16 chunks, the last one of 40 sites
    default = gpu_ctx.debug_pairscores((names, rows), table)
    assert (small == want).all() and (default == want).all()
    small = gpu_ctx.debug_pairscores((names, rows), ASYM, chunk_sites=64)
    assert (small == nj_ref.pairwise_scores_np(rows, ASYM)).all() and (small == gpu_ctx.debug_pairscores((names, rows), ASYM)).all()
    for bad in (8, 72, (1 << 20) + 16):                                              # no multiple of 16, or above the accumulator's bound
        with pytest.raises(engine.PmlError) as e:
            gpu_ctx.debug_pairscores((names, rows), table, chunk_sites=bad)
        assert e.value.code == engine.EINVAL
    with pytest.raises(engine.PmlError) as e:
        gpu_ctx.pairwise_scores((names, rows), np.full((24, 24), 128))
    assert e.value.code == engine.EINVAL


# ---- 3. bytes the Java would drop ----
@pytest.mark.parametrize("byte", ["J", "*", " "])
def test_byte_outside_the_alphabet_is_refused(gpu_ctx, byte):
    rng = np.random.default_rng(3)
    names, rows = ["alpha", "beta", "gamma_3", "delta"], _rows(rng, 4, 40)
    rows[2] = rows[2][:17] + byte + rows[2][18:]
    for call in (lambda: gpu_ctx.pairwise_scores((names, rows)), lambda: gpu_ctx.nj_tree((names, rows)),
                 lambda: gpu_ctx.nj_replicates([(names, rows)])):
        with pytest.raises(engine.PmlError) as e:
            call()
        assert e.value.code == -2                                                    # PML_EPARSE
        msg = str(e.value)
        assert "'gamma_3'" in msg and "column 17" in msg and "0x%02x" % ord(byte) in msg, msg


# ---- 4. replicates over genes with different taxon subsets ----
def _six_genes():
    rng = np.random.default_rng(44)
    taxa = ["T%02d" % i for i in range(10)]
    members = [[0, 1, 2, 3, 4, 5], [1, 2, 3, 4, 6, 7, 8], [0, 2, 4, 6, 8], [0, 1, 2, 3, 4, 5, 6, 7, 8], [3, 4, 5, 6, 7], [9, 0, 1, 5, 7, 8]]
    sites = [37, 64, 129, 200, 15, 90]
    genes = []
    for m, L in zip(members, sites):
        order = list(rng.permutation(m))                                             # every gene lists its taxa in its own order
        genes.append(([taxa[i] for i in order], _rows(rng, len(order), L)))
    return genes


GENES = _six_genes()
SELS = [[0, 1, 2], [3, 4, 5], [0, 2, 5], [1, 3, 4]]                                  # T09 occurs in gene 5 alone: replicates 0 and 3 lack it


def _restated(genes, sel, table, topology=False):
    names, rows = engine.concatenate(genes, sel)
    S = (nj_ref.pairwise_scores_np(rows, table) - 1).astype(np.float64)
    tree = nj_ref.nj_topology(names, S.tolist(), nj_ref.SIMILARITY) if topology else nj_ref.nj_tree_string(names, S.tolist(), nj_ref.SIMILARITY)
    return names, S, tree


def test_replicates_over_different_taxon_sets(gpu_ctx):
    assert sum("T09" in g[0] for g in GENES) == 1
    for table, ref in ((None, BLOSUM), (ASYM, ASYM)):
        trees, mats = gpu_ctx.nj_replicates(GENES, SELS, table=table, scores=True)
        topo = gpu_ctx.nj_replicates(GENES, SELS, table=table, form=engine.NJ_TOPOLOGY)
        sizes = []
        for r, sel in enumerate(SELS):
            names, S, want = _restated(GENES, sel, ref)
            sizes.append(len(names))
            assert mats[r].shape == S.shape and (mats[r] == S).all()
            _same_tree(trees[r], want)
            assert topo[r] == _restated(GENES, sel, ref, topology=True)[2]
        assert sizes == [9, 10, 10, 9]
        names, S, want = _restated(GENES, None, ref)
        trees, mats = gpu_ctx.nj_replicates(GENES, None, table=table, scores=True)
        assert len(trees) == 1 and (mats[0] == S).all()
        _same_tree(trees[0], want)
        assert tree_builder.buildConcatenatedNeighborJoiningTree(GENES, ctx=gpu_ctx) == _restated(GENES, None, BLOSUM, topology=True)[2]
    # one alignment through the runner: the builder's `nj` method
    r = tree_builder.NeighborJoiningRunner(gpu_ctx)
    r.setAlignment(tree_builder.SequenceAlignment(*GENES[3])); r.run()
    _same_tree(r.getResult(), nj_ref.tree_from_rows(GENES[3][0], GENES[3][1], BLOSUM))
    with pytest.raises(engine.PmlError) as e:                                        # three taxa: the Java returns null
        gpu_ctx.nj_tree((GENES[0][0][:3], GENES[0][1][:3]))
    assert e.value.code == engine.EINVAL


# ---- 5. one k_pairscore launch for the full tree and all replicates ----
def test_launch_accounting(gpu_ctx):
    before, sums_before = gpu_ctx.kernel_stats()["pairscore"], gpu_ctx.pairscore_sum_stats()["launches"]
    gpu_ctx.nj_jackknife(GENES, reps=20, seed=5)
    after = gpu_ctx.kernel_stats()["pairscore"]
    assert after["launches"] - before["launches"] == 1
    assert after["algo_bytes"] - before["algo_bytes"] == sum(len(g[0]) * len(g[1][0]) for g in GENES)
    assert gpu_ctx.pairscore_sum_stats()["launches"] - sums_before == 1              # and one k_pairscore_sum launch


# ---- 6. the jackknife end to end ----
@pytest.mark.parametrize("rule", [engine.SUPPORT_DECORATOR, engine.SUPPORT_RESTRICTED])
def test_nj_jackknife(gpu_ctx, rule):
    reps, seed = 20, 5
    r = gpu_ctx.nj_jackknife(GENES, reps=reps, seed=seed, support_rule=rule)
    main = nj_ref.strip_labels(r["newick"])
    _same_tree(main, _restated(GENES, None, BLOSUM)[2])
    draw = engine.jackknife_draw(len(GENES), reps, 0, seed)
    assert len(r["support_trees"]) == reps
    for got, sel in zip(r["support_trees"], draw):
        _same_tree(got, _restated(GENES, sel, BLOSUM)[2])
    assert any(len(decorator_ref._main_taxa(t)) < 10 for t in r["support_trees"])    # some replicate lacks T09
    labels = decorator_ref.labelled_counts(r["newick"])
    ref = decorator_ref.decorator_counts if rule == engine.SUPPORT_DECORATOR else decorator_ref.restricted_counts
    assert labels == ref(main, r["support_trees"])
    assert len(labels) == 10 - 3                                                     # every inner node of the NJ text carries a count
    assert labels == decorator_ref.labelled_counts(engine.support_tree_rule(main, r["support_trees"], rule))
    with pytest.raises(engine.PmlError) as e:                                        # not sharded
        o = engine._lib.JackknifeOpts(reps, 0, seed, 0, 0.0, 0, 2)
        import ctypes as C
        keep = []
        alns = (engine._lib.Alignment * len(GENES))(*[engine._aln_struct(g[0], g[1], keep) for g in GENES])
        a, b = C.c_void_p(), C.c_void_p()
        gpu_ctx._check(gpu_ctx.L.pml_nj_jackknife(gpu_ctx.ptr, len(GENES), alns, C.byref(o), None, rule, C.byref(a), C.byref(b)))
    assert e.value.code == engine.EINVAL


# ---- 7. the Aquificales stand-in: full NJ tree + 100 NJ support trees ----
def test_aquificales_standin_nj():
    d = json.load(open(os.path.join(GOLD, "standin_Aquificales.json")))
    genes = [(g["names"], g["rows"]) for g in d["genes"]]
    ctx = engine.Context(0, profile=True)
    try:
        reps, seed = 100, 1
        t0 = time.time()
        r = tree_builder.buildConcatenatedTreeWithGeneWiseJackKnifeSupport(genes, reps=reps, supportTreeMethod=tree_builder.NEIGHBOR_JOINING,
                                                                          fullTreeMethod=tree_builder.NEIGHBOR_JOINING, ctx=ctx, seed=seed)
        wall = time.time() - t0
        ks, ss = ctx.kernel_stats()["pairscore"], ctx.pairscore_sum_stats()
        t0 = time.time()
        main = nj_ref.strip_labels(r["newick"])
        _same_tree(main, _restated(genes, None, BLOSUM)[2])
        for got, sel in zip(r["support_trees"], engine.jackknife_draw(len(genes), reps, 0, seed)):
            _same_tree(got, _restated(genes, sel, BLOSUM)[2])
        ref_wall = time.time() - t0
        assert len(r["support_trees"]) == reps
        assert decorator_ref.labelled_counts(r["newick"]) == decorator_ref.decorator_counts(main, r["support_trees"])
        print("NJTIME Aquificales stand-in (%d genes, %d taxa, %d columns, %d replicates): k_pairscore %d launch(es) %.3f ms, k_pairscore_sum %d launch(es) %.3f ms, "
              "whole call %.1f ms, numpy restatement of the same trees %.1f ms"
              % (len(genes), len(d["taxa"]), sum(len(g[1][0]) for g in genes), reps, ks["launches"], ks["ms"], ss["launches"], ss["ms"], 1e3 * wall, 1e3 * ref_wall))
    finally:
        ctx.close()


# ---- 8. nj support trees under an ML full tree, and the tree-step tool ----
def test_nj_support_trees_for_an_ml_full_tree(gpu_ctx):
    reps, seed = 6, 5
    r = tree_builder.buildConcatenatedTreeWithGeneWiseJackKnifeSupport(GENES, reps=reps, supportTreeMethod=tree_builder.NEIGHBOR_JOINING,
                                                                      ctx=gpu_ctx, seed=seed)
    assert len(r["support_trees"]) == reps and r["lnl"] < 0
    for got, sel in zip(r["support_trees"], engine.jackknife_draw(len(GENES), reps, 0, seed)):       # the draw the other methods get
        _same_tree(got, _restated(GENES, sel, BLOSUM)[2])
    assert decorator_ref.labelled_counts(r["newick"]) == decorator_ref.decorator_counts(nj_ref.strip_labels(r["newick"]), r["support_trees"])
    with pytest.raises(ValueError):
        tree_builder.buildConcatenatedTreeWithGeneWiseJackKnifeSupport(GENES, reps=2, supportTreeMethod=tree_builder.ML,
                                                                      fullTreeMethod=tree_builder.NEIGHBOR_JOINING, ctx=gpu_ctx)


def test_tree_step_tool_with_nj_methods(gpu_ctx, tmp_path, monkeypatch):
    import sys
    monkeypatch.syspath_prepend(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import pepr_tree_step
    d = tmp_path / "alignments"
    d.mkdir()
    for i, (names, rows) in enumerate(GENES):
        (d / ("g%d.fasta" % i)).write_text("".join(">%s\n%s\n" % (n, r) for n, r in zip(names, rows)))
    run = str(tmp_path / "run")
    pepr_tree_step.main(["-run_name", run, "-alignment_dir", str(d), "-support_reps", "8", "-seed", "3",
                         "--full-tree-method", "nj"])                       # nj support trees are the default under an nj full tree
    want = gpu_ctx.nj_jackknife(GENES, reps=8, seed=3, support_rule=engine.SUPPORT_DECORATOR)
    assert open(run + ".nwk").read() == want["newick"] + "\n"
    assert open(run + ".sup").read().splitlines() == want["support_trees"]
    with pytest.raises(SystemExit):                                                  # no model to hand to nj trees
        pepr_tree_step.main(["-run_name", run, "-alignment_dir", str(d), "--full-tree-method", "nj", "--support-matrix", "PROTGAMMAWAG"])
