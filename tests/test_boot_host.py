"""The column bootstrap, host side (no GPU): the draw rule through pml_boot_draws_host -- the functions k_boot_count runs, compiled
for the host -- against the restatement (boot_ref.py) and the hand-worked anchors; the refusals; the mirror's dispatch and the tool
on a stub context; and boot_host.cpp alone under the host sanitizers."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from pepr_amd import _lib, engine, tree_builder
import boot_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "boot_cases.json")))
NEW_SYMBOLS = ["pml_bootstrap2", "pml_boot_draws_host", "pml_boot_tile", "pml_debug_boot_replicate", "pml_boot_stats", "pml_boot_replicate_lnls"]


@pytest.mark.parametrize("case", GOLD["cases"], ids=["seed%d-ncols%d-rep%d" % (c["seed"], c["ncols"], c["rep"]) for c in GOLD["cases"]])
def test_hand_worked_anchors(case):
    got = engine.boot_draws_host(case["seed"], case["rep"], case["ncols"])
    assert got.tolist() == case["draws"]
    key = ref.key_of(case["seed"], case["rep"])
    assert [ref.draw(key, j, case["ncols"]) for j in range(case["ncols"])] == case["draws"]


def test_the_issues_anchor_is_in_the_golden_file():
    by = {(c["seed"], c["ncols"], c["rep"]): c["draws"] for c in GOLD["cases"]}
    assert by[(3, 5, 0)] == [1, 4, 0, 3, 1] and by[(3, 5, 1)] == [2, 0, 0, 4, 1]


@pytest.mark.parametrize("ncols", [1, 5, 31, 1493, 2 ** 20 + 3])
@pytest.mark.parametrize("rep", [0, 1, 99])
def test_draws_host_equals_the_restatement(ncols, rep):
    seed = 3
    got = engine.boot_draws_host(seed, rep, ncols)
    assert got.dtype == np.uint32 and len(got) == ncols and int(got.max()) < ncols
    assert np.array_equal(got.astype(np.int64), ref.draws(seed, rep, ncols))          # the vectorised restatement, every draw
    key = ref.key_of(seed, rep)
    js = list(range(ncols)) if ncols <= 2000 else list(range(1000)) + list(range(ncols - 1000, ncols))   # the scalar rule: first and last 1000
    assert [int(got[j]) for j in js] == [ref.draw(key, j, ncols) for j in js]


def test_replicates_and_seeds_draw_differently():
    a, b, c = engine.boot_draws_host(3, 0, 1493), engine.boot_draws_host(3, 1, 1493), engine.boot_draws_host(4, 0, 1493)
    assert not np.array_equal(a, b) and not np.array_equal(a, c)
    assert np.array_equal(a, engine.boot_draws_host(3, 0, 1493))
    assert len(np.unique(a)) < 1493                                   # with replacement: some column is drawn twice


def test_counts_and_compaction_restatement():
    genes = [(["A", "B", "C"], ["ACCA", "ACCA", "CAAC"]), (["B", "C", "D"], ["X-?A", "ACCA", "ACCA"])]
    c2p, P = ref.col2pat(genes)
    assert c2p.tolist() == [0, 1, 1, 0, 2, 3, 3, 4] and P == 5      # X, - and ? are one code; ids continue from gene to gene
    cnt = ref.counts(genes, None, 3, 0)
    assert cnt.sum() == 8 and len(cnt) == 5
    assert ref.compact(cnt).tolist() == [p for p in range(5) if cnt[p] > 0]
    assert ref.col2pat(genes, [1])[0].tolist() == [0, 1, 1, 2]


def test_refusals():
    for rep, ncols in ((-1, 5), (0, 0), (0, -3), (0, 2 ** 31), (0, 2 ** 40)):
        with pytest.raises(engine.PmlError) as e:
            engine.boot_draws_host(3, rep, ncols)
        assert e.value.code == engine.EINVAL
    assert len(engine.boot_draws_host(3, 0, 1)) == 1 and engine.boot_draws_host(3, 0, 1)[0] == 0
    for method in (tree_builder.FAST_TREE, tree_builder.NEIGHBOR_JOINING, "upgma"):
        with pytest.raises(ValueError):
            tree_builder.buildConcatenatedTree([], 10, method, "PROTGAMMAWAG", ctx=object())
    with pytest.raises(ValueError):                                    # an unbuilt model name, before any device work
        tree_builder.buildConcatenatedTree([], 10, tree_builder.ML, "PROTGAMMAIWAG", ctx=object())
    assert engine.boot_tile() == 256


class _StubCtx:
    """stands in for a Context: the mirror and the tool call bootstrap2"""

    def __init__(self):
        self.calls = []

    def bootstrap2(self, genes, **kw):
        self.calls.append((len(genes), kw))
        topo = kw["method"] == engine.TREE_PARSIMONY
        return {"newick": "((A,B)100,C,(D,E)50);" if topo else "((A:0.1,B:0.1)100:0.1,C:0.1,(D:0.1,E:0.1)50:0.1);", "lnl": 0.0 if topo else -12.5,
                "alpha": 0.0 if topo else 0.7, "tree_length": 0.0, "npatterns": 9, "nsites": sum(len(g[1][0]) for g in genes),
                "replicates": ["((A,B),C,(D,E));"] * kw["reps"], "mp_lengths": [17] + [16] * kw["reps"] if kw["method"] != engine.TREE_ML else [-1] * (1 + kw["reps"])}

    def parsimony(self, genes, seed=0, spr_radius=20):
        self.calls.append(("parsimony", len(genes)))
        return [{"newick": "((A,B),C,(D,E));", "length": 17, "npatterns": 9} for _ in genes]


GENES = [(list("ABCDE"), ["ACDE", "ACDE", "CCDE", "CADE", "CADA"]), (list("ABCD"), ["AC", "AC", "CA", "CA"])]


def test_mirror_dispatch():
    ctx = _StubCtx()
    assert tree_builder.buildConcatenatedTree(GENES, 7, tree_builder.PARSIMONY, "PROTGAMMAWAGF", ctx=ctx, seed=9) == "((A,B)100,C,(D,E)50);"
    n, kw = ctx.calls[-1]
    assert n == 2 and kw["reps"] == 7 and kw["seed"] == 9 and kw["method"] == engine.TREE_PARSIMONY and kw["pi_mode"] == engine.PI_EMPIRICAL
    assert kw["parsimony_radius"] == 20 and kw["spr_radius"] == 5
    r = tree_builder.buildConcatenatedTree([tree_builder.SequenceAlignment(*g) for g in GENES], 0, tree_builder.ML, "PROTGAMMAWAG", ctx=ctx, details=True)
    assert ctx.calls[-1][1]["method"] == engine.TREE_ML and ctx.calls[-1][1]["reps"] == 0 and r["lnl"] == -12.5
    tree_builder.buildConcatenatedTree(GENES, 3, tree_builder.PARSIMONY_BL, "PROTGAMMAWAG", ctx=ctx)
    assert ctx.calls[-1][1]["method"] == engine.TREE_PARSIMONY_BL
    # the RAxMLRunner mirror: parsimony with bootstrapReps > 0 is `-Y -N reps` on its one alignment
    for setter, method in (("setParsimonyOnly", engine.TREE_PARSIMONY), ("setParsimonyWithBL", engine.TREE_PARSIMONY_BL)):
        ctx = _StubCtx()
        rx = tree_builder.RAxMLRunner(ctx=ctx)
        getattr(rx, setter)(True)
        rx.setBootstrapReps(4); rx.setAlignment(tree_builder.SequenceAlignment(*GENES[0]))
        rx.run()
        assert len(ctx.calls) == 1 and ctx.calls[0][0] == 1 and ctx.calls[0][1]["method"] == method and ctx.calls[0][1]["reps"] == 4
        got = rx.getParsimonyTree() if method == engine.TREE_PARSIMONY else rx.getParsimonyWithBLTree()
        assert got is not None and ")100" in got and len(rx.bootstrapTrees) == 4
    ctx = _StubCtx()                                                   # without replicates the runner builds the `-y` tree as ever
    rx = tree_builder.RAxMLRunner(ctx=ctx)
    rx.setParsimonyOnly(True); rx.setAlignment(tree_builder.SequenceAlignment(*GENES[0]))
    rx.run()
    assert ctx.calls == [("parsimony", 1)] and rx.getParsimonyTree() == "((A,B),C,(D,E));"
    # PhylogeneticTreeBuilder passes the replicates on (PhylogeneticTreeBuilder.java:136-181)
    ctx = _StubCtx()
    tbld = tree_builder.PhylogeneticTreeBuilder(ctx)
    tbld.setTreeBuildingMethod(tree_builder.PARSIMONY); tbld.setBootstrapReps(6); tbld.setAlignment(tree_builder.SequenceAlignment(*GENES[0]))
    tbld.run()
    assert ctx.calls[0][1]["reps"] == 6 and tbld.getTreeString() == "((A,B)100,C,(D,E)50);"


def test_tool_concatenated_flag(tmp_path, monkeypatch, capsys):
    d = tmp_path / "aln"
    d.mkdir()
    for k, (names, rows) in enumerate(GENES):
        (d / ("fam%d.fa" % k)).write_text("".join(">%s\n%s\n" % (t, r) for t, r in zip(names, rows)))
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import pepr_tree_step
    finally:
        sys.path.pop(0)
    ctx = _StubCtx()
    monkeypatch.setattr(pepr_tree_step.engine, "Context", lambda device=0: ctx)
    run = str(tmp_path / "run1")
    pepr_tree_step.main(["-run_name", run, "-alignment_dir", str(d), "-concatenated", "-support_reps", "3", "-seed", "4", "--full-tree-method", "parsimony"])
    assert ctx.calls[0][1]["reps"] == 3 and ctx.calls[0][1]["seed"] == 4 and ctx.calls[0][1]["method"] == engine.TREE_PARSIMONY
    assert open(run + ".nwk").read() == "((A,B)100,C,(D,E)50);\n" and open(run + ".sup").read().splitlines() == ["((A,B),C,(D,E));"] * 3
    assert "parsimony length 17" in capsys.readouterr().out
    with pytest.raises(SystemExit):
        pepr_tree_step.main(["-run_name", run, "-alignment_dir", str(d), "-concatenated", "--support-tree-method", "ml"])


def test_new_symbols_are_declared_listed_and_exported():
    header = open(os.path.join(ROOT, "include", "peprml.h")).read()
    L = _lib.load()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, header), s
        assert s in _lib.SYMBOLS, s
        assert hasattr(L, s), s
    for text in ("parity unpinned", "rapid-bootstrap shortcuts", "`-Y -N` writes are not", "PhylogenomicPipeline2.buildConcatenatedTree (:836-890)", "pml_bootstrap_opts2"):
        assert text in header, text
    hpp = open(os.path.join(ROOT, "pepr_amd", "csrc", "boot.hpp")).read()
    assert "parity unpinned" in hpp and "gs_draw" in hpp


def test_host_half_standalone_under_host_sanitizers(tmp_path):
    """boot_host.cpp is plain C++: built ALONE with a small main under AddressSanitizer and UndefinedBehaviorSanitizer and run as a
    program of its own; its draws, counts, compaction, column totals and seeds equal the restatement's"""
    exe = str(tmp_path / "boot_standalone")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", os.path.join(ROOT, "pepr_amd", "csrc", "boot_host.cpp"),
                           os.path.join(ROOT, "tests", "boot_standalone", "main.cpp"), "-o", exe])
    rng = np.random.default_rng(20261020)
    c2p = np.sort(rng.integers(0, 40, 300))
    cmds = ["draws 3 0 5", "draws 3 1 5", "draws 7 99 1493", "draws 3 0 1", "draws 3 -1 5", "draws 3 0 0", "draws 3 0 2147483648",
            "counts 11 2 40 300 " + " ".join(map(str, c2p)), "counts 11 0 1 1 0",
            "total 3 10 0 5", "total 2 2147483647 1", "total 1 0", "total 1 2147483647", "pseed 3 0", "pseed 3 5", "pseed 4294967295 1"]
    path = str(tmp_path / "cmds.txt")
    open(path, "w").write("\n".join(cmds) + "\n")
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    out = r.stdout.splitlines()
    assert len(out) == len(cmds)
    assert out[0] == "draws 1 4 0 3 1" and out[1] == "draws 2 0 0 4 1" and out[3] == "draws 0"
    assert [int(x) for x in out[2].split()[1:]] == ref.draws(7, 99, 1493).tolist()
    assert out[4] == out[5] == out[6] == "draws error -1"
    want = np.bincount(c2p[ref.draws(11, 2, 300)], minlength=40)
    counts, idx = out[7].split(" | ")
    assert [int(x) for x in counts.split()[1:]] == want.tolist() and [int(x) for x in idx.split()[1:]] == ref.compact(want).tolist()
    assert out[8] == "counts 1 | idx 0"
    assert out[9] == "total 15" and out[10].startswith("total error") and "2^31" in out[10] and out[11].startswith("total error")
    assert out[12] == "total 2147483647"
    assert out[13] == "pseed 3" and out[14] == "pseed 8" and out[15] == "pseed %d" % 0x9E3779B9
