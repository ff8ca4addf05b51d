"""The homology-search rule on the CPU: pml_sw_search_host against tests/sw_ref.py, exactly -- scores, indices and table bytes --
and its table through the filters and the clustering that follow it."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from pepr_amd import _lib, engine, tree_builder
import mcl_ref
import sw_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
NEW_SYMBOLS = ["pml_sw_search", "pml_sw_search_host", "pml_sw_result_free", "pml_sw_class_limits", "pml_debug_sw_scores", "pml_sw_stats"]
from sw_ref import NO_P, PLAIN, asym_tables, flanked, mutate, planted_families, random_protein


def one_pair(q, t, **opts):
    """the host twin's score of one pair: t alone in a genome, every hit allowed through"""
    r = engine.sw_search_host([[("t", t)], [("q", q)]], evalue=1e300, **opts)
    got = [s for qi, g, s in zip(r["query"], r["target_genome"], r["score"]) if qi == 1 and g == 0]
    return got[0] if got else 0


def check_against_ref(genomes, **opts):
    r = engine.sw_search_host(genomes, **opts)
    ropts = dict(opts)
    if "traceback" in ropts:
        ropts["traceback_"] = ropts.pop("traceback")
    e = ref.search(genomes, **ropts)
    assert e["margin"] > 1e-6                     # no winner's E so near the cutoff that libm could flip it
    assert r["table"] == e["table"]
    assert list(zip(r["query"], r["subject"], r["target_genome"], r["score"])) == [h[:4] for h in e["hits"]]
    assert r["cells"] == e["cells"]
    for b, h in zip(r["bits"], e["hits"]):
        assert abs(b - h[4]) <= 1e-12 * abs(h[4])
    return r, e


def test_symbols_and_header():
    header = open(os.path.join(ROOT, "include", "peprml.h")).read()
    L = _lib.load()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, header), s
        assert s in _lib.SYMBOLS, s
        assert hasattr(L, s), s
    for text in ("PARITY WITH blastall IS UNPINNED", "NOT BUILT", "SEG masking", "composition-based statistics", "effective-length correction",
                 "BlastRunner.java:539-599", ":1061-1077", "0.267", "0.041"):
        assert text in header, text


def test_hand_checked_scores():
    assert one_pair("AAAA", "AAAA") == 16 == ref.score("AAAA", "AAAA")
    a, b = "WWWWWHHHHH", "WWWWWAAHHHHH"
    assert ref.score(a, b) == 82 and ref.score(b, a) == 82            # 55 + 40 - 13: a gap of two, once as E and once as F
    assert one_pair(a, b) == 82 and one_pair(b, a) == 82
    assert ref.score("WWWW", "PPPP") == 0
    r = engine.sw_search_host([[("t", "PPPP")], [("q", "WWWW")]], evalue=1e300)
    assert sorted(zip(r["query"], r["subject"])) == [(0, 0), (1, 1)]  # only the self hits: no positive cell across


def test_gap_costs_and_table():
    a, b = "WWWWWHHHHH", "WWWWWAAAAHHHHH"
    for go, ge in ((11, 1), (5, 2), (1, 1), (20, 3)):
        assert one_pair(a, b, gap_open=go, gap_extend=ge) == ref.score(a, b, gap_open=go, gap_extend=ge)
    t = ref.blosum62().copy()
    t[0][0] = 9
    t[17][8] = 3                                                       # asymmetric: W against H
    assert one_pair("AAWA", "AAHA", table=t) == ref.score("AAWA", "AAHA", table=t)
    assert one_pair("AAHA", "AAWA", table=t) == ref.score("AAHA", "AAWA", table=t)


def test_asymmetric_tables_both_ways_round():
    """table[query residue][subject residue]: on tables that are not their own transpose, one of them with both ends of int8"""
    rng = np.random.default_rng(29)
    pairs = [(random_protein(rng, int(m)), random_protein(rng, int(n))) for m, n in rng.integers(1, 61, (30, 2))]
    pairs = [(q, s) if k % 2 else (q, mutate(rng, q, 0.4)) for k, (q, s) in enumerate(pairs)]    # every other pair related: mismatches inside the alignment
    for name, t in zip(("mild", "wild"), asym_tables()):
        assert (t != t.T).any() and t.min() >= -128 and t.max() <= 127
        tt = np.ascontiguousarray(t.T)
        changed = 0
        for q, s in pairs:
            want, back = ref.score(q, s, table=t), ref.score(s, q, table=t)
            assert one_pair(q, s, table=t) == want, (name, q, s)
            assert one_pair(s, q, table=t) == back, (name, s, q)
            assert ref.score(s, q, table=tt) == want and one_pair(s, q, table=tt) == want        # S(q, s, T) == S(s, q, T^T)
            changed += ref.score(q, s, table=tt) != want
        print(name, "table: the transpose changes", changed, "of", len(pairs), "scores")
        assert 2 * changed >= len(pairs)                              # the pairs tell a table from its transpose
    wild = asym_tables()[1]
    assert (wild[0][1], wild[1][0], wild[17][17]) == (127, -128, 127)
    assert one_pair("AW", "RW", table=wild) == ref.score("AW", "RW", table=wild) == 254
    assert one_pair("RW", "AW", table=wild) == ref.score("RW", "AW", table=wild) == 127


def test_gap_costs_at_the_documented_limit():
    rng = np.random.default_rng(31)
    p = random_protein(rng, 60, PLAIN)
    q, s = p, p[:30] + p[33:]                                          # three residues of the query face a gap
    big = 1 << 20
    got = {}
    for go, ge in ((big, big), (1, big), (big, 1), (1, 1)):
        got[go, ge] = ref.score(q, s, gap_open=go, gap_extend=ge)
        assert one_pair(q, s, gap_open=go, gap_extend=ge) == got[go, ge], (go, ge)
        assert one_pair(s, q, gap_open=go, gap_extend=ge) == ref.score(s, q, gap_open=go, gap_extend=ge) == got[go, ge], (go, ge)
    assert got[1, 1] > got[big, 1] == got[1, big] == got[big, big] > 0  # only the cheap gap is taken
    for opts in ({"gap_open": big + 1}, {"gap_extend": big + 1}):
        with pytest.raises(engine.PmlError) as e:
            engine.sw_search_host([[("t", s)], [("q", q)]], **opts)
        assert e.value.code == engine.EINVAL


def test_flank_identity():
    """score(flanked(core), s) == score(core, s) for s out of NO_P: what makes the expectations of very long sequences cheap"""
    rng = np.random.default_rng(37)
    total = 2000
    table = ref.blosum62()
    assert (table[ref.ORDER.index("P")][ref.encode(NO_P)] < 0).all() and (table[ref.encode(NO_P), ref.ORDER.index("P")] < 0).all()
    for n in (40, 73, 100):
        core = random_protein(rng, n)
        piece = "".join(c if c in NO_P else "A" for c in mutate(rng, core.upper(), 0.2)[5:35])
        s = random_protein(rng, 20, NO_P) + piece + random_protein(rng, 10, NO_P)                 # a relative of the core, free of P
        assert not set(s) - set(NO_P)
        want, back = ref.score(core, s), ref.score(s, core)
        assert want > 40
        for at in (0, 777, total - n):
            f = flanked(core, total, at)
            assert len(f) == total and f[at:at + n] == core
            assert ref.score(f, s) == want and one_pair(f, s) == want, (n, at)             # the flank on the query's side
            assert ref.score(s, f) == back and one_pair(s, f) == back, (n, at)             # ... and on the subject's


def test_random_proteins():
    rng = np.random.default_rng(11)
    lens = [1, 2, 70, 33] + [int(x) for x in rng.integers(1, 71, 8)]
    genomes = [[("p%d x" % i, random_protein(rng, n)) for i, n in enumerate(lens[:6])], [("r%d" % i, random_protein(rng, n)) for i, n in enumerate(lens[6:])]]
    r, _ = check_against_ref(genomes, evalue=1e6)
    assert len(r["query"]) >= 12
    check_against_ref(genomes)


def test_selection_rules():
    rng = np.random.default_rng(3)
    p, other, lone = random_protein(rng, 40), random_protein(rng, 35), random_protein(rng, 30)
    genomes = [[("a0", other), ("a1", p), ("a2", ""), ("a3", p)], [("b0 the only one", lone)], [("c0", p.lower()), ("c1", other)]]
    r, _ = check_against_ref(genomes)
    hits = set(zip(r["query"], r["subject"]))
    assert (1, 1) in hits and (3, 1) in hits and (5, 1) in hits      # two identical subjects: the lower position wins, also as the self hit's rival
    assert all((q, q) in hits for q in (0, 1, 4, 5, 6)) and (3, 3) not in hits
    assert 2 not in r["query"] and 2 not in r["subject"]              # the empty protein is neither query nor subject
    assert r["target_genome"] == sorted(r["target_genome"])           # target by target ...
    for g in range(3):
        qs = [q for q, t in zip(r["query"], r["target_genome"]) if t == g]
        assert qs == sorted(qs)                                       # ... the queries in genome order, then file order


def test_evalue_cutoff_sides():
    genomes = [[("t", "WWWWHW")], [("q", "WWWW")]]
    e = [h for h in ref.search(genomes, evalue=1e300)["hits"] if h[0] == 1 and h[2] == 0][0][5]
    for cutoff, expect in ((2.0 * e, True), (0.5 * e, False)):
        assert ref.search(genomes, evalue=cutoff)["margin"] > 1e-6
        r, _ = check_against_ref(genomes, evalue=cutoff)
        assert ((1, 0) in set(zip(r["query"], r["subject"]))) == expect


def test_invalid_input():
    for genomes, opts in (([[("a", "AC-A")]], {}), ([[("a", "A" * 65536)]], {}), ([[("a", "ACA")]], {"hits_per_query": 2}), ([[("a", "AC*")]], {}),
                          ([[("a", "ACA")]], {"gap_open": -1})):
        with pytest.raises(engine.PmlError) as e:
            engine.sw_search_host(genomes, **opts)
        assert e.value.code == engine.EINVAL
    assert engine.sw_search_host([[("a", "")], []])["query"] == []
    assert engine.sw_search_host([])["table"] == b""


def test_traceback():
    a, b = "WWWWWHHHHH", "WWWWWAAHHHHH"
    assert ref.traceback(a, b) == ("83.33", 12, 0, 1, 1, 10, 1, 12)
    assert ref.traceback(b, a) == ("83.33", 12, 0, 1, 1, 12, 1, 10)
    # two co-optimal end cells: WW ends at subject 2 and at subject 5; the first in row-major order wins
    assert ref.traceback("WW", "WWPWW") == ("100.00", 2, 0, 0, 1, 2, 1, 2)
    rng = np.random.default_rng(8)
    p = random_protein(rng, 50, "ARNDCQEGHILKMFPSTWYV")
    genomes = [[("t0", b), ("t2", p[:20] + p[24:])], [("t1", "WWPWW")], [("q0", a), ("q1", "WW"), ("q2", p)]]
    r, _ = check_against_ref(genomes, traceback=True, evalue=10.0)
    lines = [ln.split("\t") for ln in r["table"].decode().splitlines()]
    assert ["q0", "t0", "83.33", "12", "0", "1", "1", "10", "1", "12"] in [ln[:10] for ln in lines]
    assert ["q1", "t1", "100.00", "2", "0", "0", "1", "2", "1", "2"] in [ln[:10] for ln in lines]
    assert all(len(ln) == 12 for ln in lines)


def test_table_feeds_the_homolog_group_step():
    genomes = planted_families()
    r, _ = check_against_ref(genomes)
    table = r["table"].decode()
    filtered = engine.hits_filter_host(table)
    assert len(filtered.splitlines()) == len(table.splitlines())
    bidir = engine.hits_bidirectional_host(table, 11)
    assert bidir
    labels, arcs = mcl_ref.parse_abc(filtered)
    clusters = engine.mcl_cluster_host(len(labels), arcs)["clusters"]
    assert sorted(sorted(labels[i] for i in c) for c in clusters) == [sorted("g%d_f%d" % (g, f) for g in range(3)) for f in range(3)]


def test_host_half_standalone_under_host_sanitizers(tmp_path):
    """sw_host.cpp is plain C++: built ALONE (with nj.cpp, the table) and a small main under AddressSanitizer and
    UndefinedBehaviorSanitizer and run as a program of its own on random sets, empty proteins and genomes, and a bad byte"""
    exe = str(tmp_path / "sw_standalone")
    src = os.path.join(ROOT, "pepr_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", os.path.join(src, "sw_host.cpp"), os.path.join(src, "nj.cpp"),
                           os.path.join(ROOT, "tests", "sw_standalone", "main.cpp"), "-o", exe])
    rng = np.random.default_rng(17)
    base = [random_protein(rng, int(n)) for n in rng.integers(1, 90, 7)]
    genomes = [[("a%d" % i, s) for i, s in enumerate(base[:4] + [""])], [], [("b%d" % i, s[:-3] + s[-1:]) for i, s in enumerate(base)]]
    text = "".join("G\n" + "".join("P %s %s\n" % p for p in g) for g in genomes)
    for tb, cutoff in ((0, 0.1), (1, 10.0)):
        want = engine.sw_search_host(genomes, traceback=bool(tb), evalue=cutoff)
        out = subprocess.run([exe, str(tb), repr(cutoff)], input=text.encode(), capture_output=True, check=True).stdout
        head, _, table = out.partition(b"\n")
        assert head == b"rc 0 hits %d cells %d" % (len(want["query"]), want["cells"]) and table == want["table"]
    for bad in ("G\nP x AC-D\n", "G\nP x " + "A" * 65536 + "\n"):
        assert subprocess.run([exe], input=bad.encode(), capture_output=True, check=True).stdout.startswith(b"rc -1 ")
    assert subprocess.run([exe], input=b"", capture_output=True, check=True).stdout == b"rc 0 hits 0 cells 0\n"


def test_tools_and_mirror_class(tmp_path):
    import pepr_homolog_groups
    import pepr_homology_search
    assert callable(pepr_homology_search.main) and pepr_homolog_groups.BLAST == "blast"
    faa = tmp_path / "g.faa"
    faa.write_text(">p1 first protein [taxon a]\nMKV\nA\n\nLL\n>\n>p2\nW\nACD\r\n")
    # createConcatenatedSet drops lines of length <= 1: the lone A, the empty line, the bare '>' and the lone W
    assert tree_builder.HomologySearch.readGenome(str(faa)) == [("p1 first protein [taxon a]", "MKVLL"), ("p2", "ACD")]
    lim = engine.sw_class_limits()
    assert lim["lanes"] == [16, 32, 64] and lim["rows"] == [n * lim["strip"] for n in lim["lanes"]] and lim["chunk"] >= 1024
