"""Tree-set comparison, host side: the restatement (tests/treecmp_ref.py) against hand-worked cases, the closed form the device
path uses against real sets, the record builder of treecmp.cpp as a stand-alone program under the host sanitizers, the pruning
mirror, and the tool end to end on a stub context.  No device is needed."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import treecmp_ref as ref
from pepr_amd import _lib, engine, tree_builder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "treecmp_cases.json")))
NEW_SYMBOLS = ["pml_tree_compare", "pml_tree_compare_one", "pml_tree_compare_result_free", "pml_debug_tree_splits", "pml_tree_splits_free",
               "pml_debug_tree_pair_sums"]


def golden_value(x):
    return float("nan") if x["value"] == "nan" else float.fromhex(x["value"])


def same_double(a, b):
    """bit equality, every NaN taken as one value (as Java's doubleToLongBits does)"""
    return (a != a and b != b) or np.float64(a).view(np.int64) == np.float64(b).view(np.int64)


@pytest.mark.parametrize("case", GOLDEN["cases"], ids=[c["name"] for c in GOLDEN["cases"]])
def test_restatement_gives_the_hand_worked_values(case):
    s = ref.TreeSet([case["tree1"], case["tree2"]], case.get("use_lengths", True))
    rf_legacy, rf_bip, rf_splits, bd, dd = s.pair(0, 1)
    assert (rf_legacy, rf_bip, rf_splits) == (case["rf_legacy"], case["rf_bipartition"], case["rf_splits"])
    assert same_double(bd, golden_value(case["branch_dist"])), (bd, case["branch_dist"])
    assert same_double(dd, golden_value(case["discrepant_dist"])), (dd, case["discrepant_dist"])
    if case["branch_dist"]["r"] is not None:                        # the sums the hand calculation ends with
        r, ss1, ss2 = ref.branch_distance_sums(s.trees[0], s.trees[1])
        assert (r, ss1 + ss2) == (case["branch_dist"]["r"], case["branch_dist"]["den"])
    if case["discrepant_dist"]["r"] is not None:
        r, ss1, ss2 = ref.discrepant_distance_sums(s.trees[0], s.trees[1])
        assert (r, ss1 + ss2) == (case["discrepant_dist"]["r"], case["discrepant_dist"]["den"])


@pytest.mark.parametrize("case", GOLDEN["repeated"], ids=[c["name"] for c in GOLDEN["repeated"]])
def test_restatement_repeated_split_takes_the_later_branch(case):
    a = ref.JTree.from_branches(case["leaves"], case["branches1"])
    b = ref.JTree.from_branches(case["leaves"], case["branches2"])
    assert ref.robinson_foulds_legacy(a, b) == case["rf_legacy"]
    r, ss1, ss2 = ref.branch_distance_sums(a, b)
    assert (r, ss1 + ss2) == (case["branch_dist"]["r"], case["branch_dist"]["den"])
    r, ss1, ss2 = ref.discrepant_distance_sums(a, b)
    assert (r, ss1 + ss2) == (case["discrepant_dist"]["r"], case["discrepant_dist"]["den"])
    assert same_double(ref.branch_distance(a, b), golden_value(case["branch_dist"]))
    assert same_double(ref.discrepant_distance(a, b), golden_value(case["discrepant_dist"]))


def test_refused_models():
    for text in ("(A,B,C,D);", "((A,B),(C));", "((A,B),C,(D,A));", "A;"):
        with pytest.raises(ValueError):
            ref.JTree(text)
    with pytest.raises(ValueError):
        ref.TreeSet(["((A,B),C,D);", "((A,B),C,E);"])


@pytest.mark.parametrize("n,T,seed", [(4, 6, 1), (7, 40, 2), (16, 40, 3), (40, 24, 4)])
def test_closed_form_equals_the_sets(n, T, seed):
    """the device path computes the two Java RF values from counts of distinct and shared splits; here the same counts are taken
    from real sets and the closed form (derived in treecmp_ref.rf_closed_form) must give what the sets give, for pairs that share
    anything from no non-trivial split to all of them"""
    texts = ref.draw_set(n, T, seed)
    s = ref.TreeSet(texts)
    shared_seen = set()
    for i in range(T):
        for j in range(i + 1, T):
            sh, sh_nt, da, da_nt, db, db_nt = ref.pair_counts(s.trees[i], s.trees[j])
            assert ref.rf_closed_form(da, db, sh) == ref.robinson_foulds_legacy(s.trees[i], s.trees[j])
            assert ref.rf_closed_form(da_nt, db_nt, sh_nt) == ref.robinson_foulds_bipartition(texts[i], texts[j])
            shared_seen.add((sh_nt, min(da_nt, db_nt)))
    assert any(a == 0 for a, _ in shared_seen) and any(a == b and b > 0 for a, b in shared_seen)      # nothing shared ... everything shared
    if n >= 7:
        assert len({a for a, _ in shared_seen}) >= 3


def test_record_builder_standalone_under_host_sanitizers(tmp_path):
    """treecmp.cpp and host.cpp's Newick reader are plain C++: built alone with a small main under AddressSanitizer and
    UndefinedBehaviorSanitizer and run as a program of their own; its records equal the restatement's in branch order, split
    words, lengths, normalisation and flags, at sizes on both sides of every word boundary"""
    exe = str(tmp_path / "treecmp_standalone")
    src = os.path.join(ROOT, "pepr_amd", "csrc")
    # -O0: host.cpp is the whole host library, and compiling it is most of this test's time
    subprocess.check_call(["g++", "-O0", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", os.path.join(src, "treecmp.cpp"),
                           os.path.join(src, "host.cpp"), os.path.join(ROOT, "tests", "treecmp_standalone", "main.cpp"), "-o", exe])

    def run(texts, use_lengths):
        path = str(tmp_path / "trees.txt")
        with open(path, "w") as f:
            f.write("\n".join(texts) + "\n")
        r = subprocess.run([exe, path, "1" if use_lengths else "0"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "ERROR" not in r.stderr, (r.stdout[-2000:], r.stderr[-2000:])
        return r.stdout.splitlines()

    for n, T, use_lengths in [(4, 6, True), (5, 9, False), (63, 7, True), (64, 7, True), (65, 7, True), (129, 6, True), (257, 6, True), (512, 6, True)]:
        texts = ref.draw_set(n, T, 11)
        lines = run(texts, use_lengths)
        assert lines[0] == "n %d words %d" % (n, 1 if n <= 64 else 2 if n <= 128 else 4 if n <= 256 else 8)
        at = 1
        for t, text in enumerate(texts):
            want = ref.records(text, use_lengths)
            nreal = sum(1 for w in want if w[3] & ref.REAL)
            head = lines[at].split()
            assert head[:6] == ["tree", str(t), "nreal", str(nreal), "nrec", str(len(want))], (n, t, lines[at])
            assert same_double(float.fromhex(head[7]), ref.JTree(text, use_lengths).max_length())
            for k, w in enumerate(want):
                flags, length, lnorm, words = lines[at + 1 + k].split()
                assert int(words, 16) == w[0] and int(flags) == w[3] & ~ref.LAST, (n, t, k)         # TC_LAST is the device's to set
                assert same_double(float.fromhex(length), w[1]) and same_double(float.fromhex(lnorm), w[2]), (n, t, k)
            at += 1 + len(want)
        assert at == len(lines)
    # the refusals are decided here, on the host, before anything is launched
    base = ref.draw_set(6, 2, 3)
    for bad, code in [(["((A,B),C,D);", "((A,B),C,E);"], -1), (["(A,B,C,D);"], -1), (["((A,B),(C),D);"], -1), (["((A,B),C,(D,A));"], -1),
                      ([base[0], "((t000,t001"], -2), ([ref.to_newick(ref.random_tree(np.random.default_rng(1), ["x%d" % i for i in range(513)]), lengths=False)], -1)]:
        out = run(bad, True)
        assert out[0].startswith("refused %d " % code), out[0]
        assert len(out[0].split(" ", 2)[2]) > 10


def _numbers_as_doubles(text):
    return re.sub(r":([0-9.eE+-]+)", lambda m: ":" + repr(float(m.group(1))), text)


@pytest.mark.parametrize("case", GOLDEN["prune"], ids=[c["name"] for c in GOLDEN["prune"]])
def test_remove_taxon_mirror(case):
    """BasicTree.removeTaxon + getTreeString against texts worked by hand from the Java; the fixture spells numbers as Java does
    (4.0), the project as the shortest text (4), so both sides are compared with their numbers read as doubles"""
    t = tree_builder.BasicTree(case["tree"])
    t.removeTaxon(case["remove"])
    assert _numbers_as_doubles(t.getTreeString(True, True)) == _numbers_as_doubles(case["expect"])


def test_prune_to_common_taxa():
    trees = ["((A:1,B:2):3,C:4,(D:5,X:1):2);", "((A:1,E:2):3,C:4,(D:5,B:1):2);", "(A:1,B:1,(C:1,D:1):1);"]
    pruned, removed = tree_builder.pruneToCommonTaxa(trees)
    assert removed == [(0, "X"), (1, "E")]
    for p in pruned:
        assert sorted(ref.JTree(p).leaves) == ["A", "B", "C", "D"]
    # X's sister D takes the summed length 5 + 2; E's sister A takes 1 + 3
    assert _numbers_as_doubles(pruned[0]) == _numbers_as_doubles("(C:4.0,D:7.0,(A:1.0,B:2.0):3.0);")
    assert _numbers_as_doubles(pruned[1]) == _numbers_as_doubles("(C:4.0,A:4.0,(D:5.0,B:1.0):2.0);")
    out, removed = tree_builder.pruneToCommonTaxa(trees[2:], outgroupTaxa=["D"])
    assert removed == [] and sorted(ref.JTree(out[0]).leaves) == ["A", "B", "C"]


class StubContext:
    """answers Context.tree_compare from the restatement"""

    def __init__(self):
        self.calls = []

    def tree_compare(self, newicks, window=0, use_lengths=True, want=None):
        self.calls.append((list(newicks), window, use_lengths, want))
        r = ref.TreeSet(newicks, use_lengths).compare_all(window)
        return {k: v for k, v in r.items() if want is None or k in want}


def _run_tool(argv, ctx):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import pepr_tree_compare
    finally:
        sys.path.pop(0)
    lines = []
    assert pepr_tree_compare.main(argv, ctx=ctx, out=lines.append) == 0
    return lines


def test_tool_prints_the_java_lines(tmp_path):
    a, b = tmp_path / "a.nwk", tmp_path / "b.nwk"
    a.write_text("((A:1,B:1):1,C:1,D:1);\n\n((A:1,C:1):1,B:1,(D:1,X:2):3);\n")
    b.write_text("((A:1,B:1):1,C:1,D:1);\n")
    ctx = StubContext()
    lines = _run_tool(["-tree_file", str(a), str(b)], ctx)
    assert lines[:2] == ["treeFile 0: %s" % a, "treeFile 1: %s" % b]
    assert lines[2:4] == ["tree 1 removing taxon: X", "done parsing"]
    # tree 1 after pruning: D takes 1 + 3 = 4; against tree 0: maximum 1 and 4
    d01 = ref.TreeSet(ctx.calls[0][0]).pair(0, 1)
    assert lines[4] == "0 vs 1: 1"
    assert lines[5] == "Tree Distance: 0 vs 1\t RF: 1\tBranch Dist: %s\t\t%s" % (engine.format_double(d01[3]), engine.format_double(d01[4]))
    assert lines[6] == "0 vs 2: 0" and lines[7] == "Tree Distance: 0 vs 2\t RF: 0\tBranch Dist: 0\t\t0"
    assert lines[8] == "1 vs 2: 1" and len(lines) == 10
    assert ctx.calls[0][2] is True and ctx.calls[0][3] is None
    # -use_lengths false: NaN as Java prints it; -tree_dist false: the RF lines alone
    lines = _run_tool(["-tree_file", str(b), str(b), "-use_lengths", "false"], StubContext())
    assert lines[-1] == "Tree Distance: 0 vs 1\t RF: 0\tBranch Dist: NaN\t\tNaN"
    ctx = StubContext()
    lines = _run_tool(["-tree_file", str(a), "-tree_dist", "false"], ctx)
    assert lines[-1] == "0 vs 1: 1" and ctx.calls[0][3] == ["rf_legacy"]
    assert _run_tool(["-tree_file", str(a), "-rf", "false"], StubContext())[-1] == "done parsing"


def test_format_double_reads_back():
    rng = np.random.default_rng(5)
    for x in list(rng.random(200)) + [0.0, 1.0, 0.1, 1e-300, 123456789.125, 2.0 / 3.0]:
        s = engine.format_double(x)
        assert float(s) == x and len(s) <= len(repr(float(x))) + 2
    assert engine.format_double(0.0) == "0" and engine.format_double(float("nan")) == "NaN"


def test_new_symbols_are_declared_listed_and_exported():
    header = open(os.path.join(ROOT, "include", "peprml.h")).read()
    L = _lib.load()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, header), s
        assert s in _lib.SYMBOLS, s
        assert hasattr(L, s), s
    assert "PML_K_TREEPAIRS = 13" in header and "PML_K_END = 14" in header
    assert engine.KERNELS["treepairs"] == 13
    for name in ("compareAllvsAll", "compareSlidingWindow", "rollingComparison", "getBranchDistance", "getDiscrepantBranchDistance"):
        assert callable(getattr(tree_builder, name))


def test_pair_kernel_has_no_fused_multiply_add(tmp_path):
    """the sums must round as the Java's do: a multiply, then an add.  treecmp.hip switches contraction off for the file; the
    device code of the file, compiled alone for gfx950, holds no double-precision fused multiply-add"""
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    asm = str(tmp_path / "treecmp.s")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-x", "hip", os.path.join(ROOT, "pepr_amd", "csrc", "treecmp.hip"),
                           "--offload-device-only", "-S", "-o", asm], stderr=subprocess.DEVNULL)
    text = open(asm).read()
    assert "k_tree_pairs" in text and "v_mul_f64" in text and "v_add_f64" in text
    assert "v_fma_f64" not in text and "v_fmac_f64" not in text
