"""The homolog-group rule on the CPU: tests/mcl_ref.py and pml_mcl_cluster_host against the recorded output of mcl 09-308
(tests/golden/mcl_cases.json), and the Java's filters and set selection on hand-worked cases."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from pepr_amd import _lib, engine, tree_builder
import mcl_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "mcl_cases.json")))["cases"]
NEW_SYMBOLS = ["pml_mcl_cluster", "pml_mcl_cluster_host", "pml_homolog_groups", "pml_homolog_groups_result_free", "pml_hits_filter_host",
               "pml_hits_bidirectional_host", "pml_homolog_select_host", "pml_mcl_class_limits", "pml_debug_mcl_steps", "pml_mcl_stats"]


def lines_of(labels, clusters):
    return ["\t".join(labels[i] for i in c) for c in clusters]


def test_symbols_and_header():
    header = open(os.path.join(ROOT, "include", "peprml.h")).read()
    L = _lib.load()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, header), s
        assert s in _lib.SYMBOLS, s
        assert hasattr(L, s), s
    for text in ("mcl 09-308", "-S 1100 -R 1400 -pct 90", "NOT BUILT", "sparse expansion", "PhyloPipeline.java:357-406", ":911-987", ":989-1024",
                 "a mirror with a max", "Float.toString", "NOT\n * reproduced"):
        assert text in header, text


def test_golden_cases_cover_the_issue():
    assert 10 <= len(GOLD) <= 16 and all(c["n"] <= 130 for c in GOLD)
    assert {c["inflation"] for c in GOLD} >= {1.2, 1.5, 2.0, 3.0}
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "mcl_cases.json")) < 200 * 1024


@pytest.mark.parametrize("case", GOLD, ids=[c["name"] for c in GOLD])
def test_ref_reproduces_mcl(case):
    assert ref.mcl_lines(case["abc"], np.float64, inflation=case["inflation"]) == case["lines"]
    assert ref.mcl_lines(case["abc"], np.float32, inflation=case["inflation"]) == case["lines"]


@pytest.mark.parametrize("case", GOLD, ids=[c["name"] for c in GOLD])
def test_host_twin_reproduces_mcl(case):
    labels, arcs = ref.parse_abc(case["abc"])
    r = engine.mcl_cluster_host(len(labels), arcs, inflation=case["inflation"])
    assert lines_of(labels, r["clusters"]) == case["lines"]
    assert r["iterations"] == ref.mcl_clusters(len(labels), arcs, inflation=case["inflation"])[2]


def test_host_twin_edges():
    assert engine.mcl_cluster_host(0, [])["clusters"] == []
    assert engine.mcl_cluster_host(3, [(1, 1, 5.0)])["clusters"] == [[0], [1], [2]]           # a self hit only makes a node
    assert engine.mcl_cluster_host(2, [(0, 1, 2.0), (0, 1, 7.0), (1, 0, 3.0)])["clusters"] == [[0, 1]]
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(engine.PmlError) as e:
            engine.mcl_cluster_host(2, [(0, 1, bad)])
        assert e.value.code == engine.EINVAL
    r = engine.mcl_cluster_host(4, [(0, 1, 1.0), (1, 2, 1.0), (2, 3, 1.0)], max_iter=1)
    assert r["iterations"] == 1


def test_rule_is_sensitive_to_the_mirror():
    """the committed cases tell the max-combined mirror from a sum: at least one case changes"""
    changed = 0
    for case in GOLD:
        labels, arcs = ref.parse_abc(case["abc"])
        n = len(labels)
        G = np.zeros((n, n))
        for a, b, w in arcs:
            if a != b:
                G[a, b] += w
                G[b, a] += w
        cl = []
        for comp in ref.components(G):
            c, _ = ref.mcl_component(ref.start_matrix(G[np.ix_(comp, comp)]), case["inflation"])
            cl += [[comp[i] for i in x] for x in c]
        changed += lines_of(labels, ref.order_clusters(cl)) != case["lines"]
    assert changed >= 1


# ---- filterForBidirectional, PhyloPipeline.java:911-987 ----
def m8(a, b, score, fields=12):
    f = [a, b, "90.0", "100", "3", "0", "1", "100", "1", "100", "1e-50", score]
    return "\t".join(f[:fields])


BIDIR_TABLE = "\n".join([
    m8("A", "B", "56.2"),            # first sighting of {A, B}: stored (:958-961)
    m8("C", "D", "182"),             # {C, D} is seen once only: never written
    m8("B", "A", "182"),             # second sighting: two lines (:962-973), the pair is forgotten
    m8("A", "B", "1.234e+04"),       # third sighting stores again ...
    m8("E", "E", "77"),              # a self pair, first sighting (IntPair.java:12-21 makes no exception)
    m8("X", "Y", "50", fields=11),   # 11 fields: not more than scoreField (:951), ignored
    m8("B", "A", "9"),               # ... and the fourth completes it: Float.toString(12340.0f)
    m8("E", "E", "78.5"),            # the self pair completes
    "",
]) + "\n"
BIDIR_EXPECTED = "B\tA\t182\nA\tB\t56.2\n" "B\tA\t9\nA\tB\t12340.0\n" "E\tE\t78.5\nE\tE\t77.0\n"


def test_bidirectional_filter_hand_worked():
    assert ref.filter_bidirectional(BIDIR_TABLE) == BIDIR_EXPECTED
    assert engine.hits_bidirectional_host(BIDIR_TABLE) == BIDIR_EXPECTED


def test_float_to_string():
    """Float.toString through the second line of a completed pair (:968)"""
    for text, want in (("56.2", "56.2"), ("182", "182.0"), ("1.234e+04", "12340.0"), ("0.00012", "1.2E-4"), ("1e7", "1.0E7"), ("12345678", "1.2345678E7"),
                       ("0.001", "0.001"), ("9999999", "9999999.0"), ("0.1", "0.1"), ("3.4028235e38", "3.4028235E38"), ("nan", "NaN"), ("1e39", "Infinity"),
                       ("-inf", "-Infinity"), ("-0", "-0.0")):
        table = m8("A", "B", text) + "\n" + m8("B", "A", "1") + "\n"
        assert ref.java_float_to_string(float(text)) == want
        assert engine.hits_bidirectional_host(table) == "B\tA\t1\nA\tB\t%s\n" % want, text


def test_hit_pair_filter():
    """filterHitPairFile :989-1024: fields 0, 1, 11 of the lines with more than one field"""
    table = m8("A", "B", "56.2") + "\n\nsingle\n" + m8("C", "D", "1e-3") + "\textra\n"
    want = "A\tB\t56.2\nC\tD\t1e-3\n"
    assert ref.filter_hit_pairs(table) == want
    assert engine.hits_filter_host(table) == want
    with pytest.raises(engine.PmlError):                   # the Java's ArrayIndexOutOfBoundsException at :1010
        engine.hits_filter_host(m8("A", "B", "1", fields=5) + "\n")


# ---- the set selection, SequenceSetProviderImpl.java and PhylogenomicPipeline2.java:564-605 ----
CLUSTERS = [[0, 1, 2, 3, 4], [5, 6, 7, 8], [9, 10, 11, 12], [13, 14, 15], [16, 17], [18]]
TAXON = [0, 1, 2, 3, 4,  0, 1, 2, 2,  0, 1, 2, 3,  0, 1, 2,  0, 0,  5]          # cluster 1 and cluster 4 hold a taxon twice


@pytest.mark.parametrize("args, want", [
    ((2, 5, False, 0, 0), [0, 1, 2, 3, 4]),            # :126-127 the size window is a sequence count: the singleton goes
    ((2, 4, False, 0, 0), [1, 2, 3, 4]),
    ((2, 5, True, 0, 0), [0, 2, 3]),                   # :223-247 rep_only drops the sets with a repeated taxon
    ((2, 5, False, 5, 2), [0, 2]),                     # :583-597 t = 3: 4 sets >= 2 -> drop; t = 4: {0, 2} >= 2 -> drop; t = 5: 1 < 2, the loop goes on without dropping
    ((2, 5, False, 3, 4), [0, 1, 2, 3]),               # t = 3: sets with >= 3 taxa are 0, 1, 2, 3 = 4 >= 4 -> drop set 4; stops at target_ntax
    ((2, 5, False, 5, 5), [0, 1, 2, 3, 4]),            # :580 not MORE than target_min_gene sets: nothing is dropped
    ((2, 5, False, 5, 9), [0, 1, 2, 3, 4]),
])
def test_set_selection_hand_worked(args, want):
    assert ref.select_sets(CLUSTERS, TAXON, *args) == want
    assert engine.homolog_select_host(CLUSTERS, TAXON, *args) == want


def test_class_limits():
    packed, lds, tile = engine.mcl_class_limits()
    assert 1 <= packed < lds and tile >= 16 and tile % 16 == 0


def test_tool_and_mirror_class_names_are_importable():
    import pepr_homolog_groups
    assert callable(pepr_homolog_groups.main) and hasattr(tree_builder, "HomologGroups")
    assert tree_builder.readFastaRecords.__doc__


def test_host_half_standalone_under_host_sanitizers(tmp_path):
    """mcl_host.cpp is plain C++: built ALONE with a small main under AddressSanitizer and UndefinedBehaviorSanitizer and run as a
    program of its own on the committed cases, random graphs (self arcs, repeats, isolated nodes, max_iter = 1) and odd tables"""
    exe = str(tmp_path / "mcl_standalone")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", os.path.join(ROOT, "pepr_amd", "csrc", "mcl_host.cpp"),
                           os.path.join(ROOT, "tests", "mcl_standalone", "main.cpp"), "-o", exe])
    rng = np.random.default_rng(8)
    graphs = []
    for case in GOLD:
        labels, arcs = ref.parse_abc(case["abc"])
        graphs.append((len(labels), arcs, case["inflation"], 0))
    for n in (1, 2, 7, 40, 300):
        m = int(rng.integers(0, 3 * n + 1))
        arcs = [(int(rng.integers(0, n)), int(rng.integers(0, n)), float(rng.integers(1, 300))) for _ in range(m)]
        graphs.append((n, arcs, 2.0, 1 if n == 40 else 0))
    graphs.append((0, [], 0.0, 0))
    text = "".join("G %d %d %r %d\n" % (n, len(arcs), infl, mi) + "".join("%d %d %r\n" % a for a in arcs) for n, arcs, infl, mi in graphs)
    tables = [BIDIR_TABLE, "", "\n\n", "a\tb", "\t\t\t\n", m8("A", "B", "nan") + "\n" + m8("B", "A", "-0") + "\n" + m8("A", "B", "x", fields=3)]
    for t in tables:
        text += "B 11 %d\n%s" % (len(t.encode()), t) + "F %d\n%s" % (len(t.encode()), t)
    out = subprocess.run([exe], input=text.encode(), capture_output=True, timeout=120)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    got = out.stdout.decode().split("\n")
    for (n, arcs, infl, mi), line in zip(graphs, got):
        want = engine.mcl_cluster_host(n, arcs, inflation=infl, max_iter=mi)
        assert line.split() == ["C", str(want["iterations"]), str(len(want["clusters"]))] + [str(int(c)) for c in want["cluster_of"]]
    rest = "\n".join(got[len(graphs):])
    want = ""
    for t in tables:
        want += engine.hits_bidirectional_host(t) + ".\n"
        try:
            want += engine.hits_filter_host(t) + ".\n"
        except engine.PmlError:
            want += "EINVAL\n.\n"
    assert rest == want
