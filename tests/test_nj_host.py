"""The host half of the reference's `nj` tree-building method (pepr_amd/csrc/nj.cpp) against its line-by-line restatement
tests/nj_ref.py: the BLOSUM62 table as the Java's loader leaves it, TreeBuilder.getNJTreeString / getNJTopology on seeded random
matrices (text structure equal, every length the same 8 bytes), the worked cases of tests/golden/nj_cases.json, the refusals,
and one run of the same source under the host sanitizers as a stand-alone program.  No device is needed."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

from pepr_amd import engine
import nj_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
FIX = json.load(open(os.path.join(GOLD, "blosum62_as_loaded.json")))
CASES = json.load(open(os.path.join(GOLD, "nj_cases.json")))["cases"]


def same_tree(got, want):
    gs, gl = nj_ref.split_tree(got)
    ws, wl = nj_ref.split_tree(want)
    assert gs == ws, (got, want)
    assert gl == wl, (got, want)


def test_table_is_the_fixture_and_has_the_loaders_quirks():
    t = engine.blosum62_as_loaded()
    assert t.shape == (24, 24) and (t == np.array(FIX["table"])).all()
    code = {c: i for i, c in enumerate(FIX["codes"])}
    assert t[code["Z"], code["Z"]] == 3           # code Z reads the file's J line: J.J = 3 (the file's Z.Z is 4)
    assert t[code["Z"], code["E"]] == -3          # J.E = -3 (the file's Z.E is 4)
    assert t[code["X"], code["X"]] == 4           # code X reads the file's Z line: Z.Z = 4 (the file's X.X is -1)
    assert t[code["X"], code["A"]] == -1          # Z.A
    assert (t[23, :] == 0).all() and (t[:, 23] == 0).all()      # gap . anything = 0
    assert (t == t.T).all()
    assert FIX["quirks"] == {"Z.Z": 3, "Z.E": -3, "X.X": 4, "X.A": -1, "gap.A": 0}


def _random_matrices():
    rng = np.random.default_rng(20261019)
    out = []
    for k in range(400):
        n = int(rng.integers(4, 41)) if k >= 8 else (4, 5, 6, 7, 8, 39, 40, 4)[k]
        kind = k % 4
        if kind == 0:
            m = rng.integers(0, 4, (n, n)).astype(float)                  # integer-valued, nearly everything ties
        elif kind == 1:
            m = rng.integers(-1000, 1000, (n, n)).astype(float)
        elif kind == 2:
            m = rng.random((n, n)) * 10.0 ** rng.integers(-3, 6)             # arbitrary doubles
        else:
            m = np.round(rng.normal(0, 3, (n, n)), 1)                        # doubles that are no binary fractions, with ties
        if k % 5:
            m = np.triu(m) + np.triu(m, 1).T                                 # symmetric, as the pipeline's matrices are
        out.append((["n%d" % i for i in range(n)], m))
    return out


RANDOM = _random_matrices()


@pytest.mark.parametrize("matrix_type", [nj_ref.DISTANCE, nj_ref.SIMILARITY])
@pytest.mark.parametrize("form", [engine.NJ_TREE, engine.NJ_TOPOLOGY])
def test_nj_from_matrix_equals_the_restatement(matrix_type, form):
    """400 seeded matrices, each under this matrix type and form; structure equal, every length bit for bit"""
    negative = 0
    for names, m in RANDOM:
        got = engine.nj_from_matrix(names, m, matrix_type, form)
        rows = m.tolist()
        want = nj_ref.nj_tree_string(names, rows, matrix_type) if form == engine.NJ_TREE else nj_ref.nj_topology(names, rows, matrix_type)
        same_tree(got, want)
        negative += any(struct.unpack("<d", x)[0] < 0 for x in nj_ref.split_tree(got)[1])
    if form == engine.NJ_TREE:
        assert negative > 0            # the unclamped last lengths do occur among the cases


def test_refusals():
    names = ["a", "b", "c", "d"]
    m = np.arange(16.0).reshape(4, 4)
    for n in (0, 1, 2, 3):
        with pytest.raises(engine.PmlError) as e:
            engine.nj_from_matrix(names[:n], m[:n, :n], nj_ref.DISTANCE, engine.NJ_TREE)
        assert e.value.code == engine.EINVAL
        with pytest.raises(engine.PmlError) as e:
            engine.nj_from_matrix(names[:n], m[:n, :n], nj_ref.SIMILARITY, engine.NJ_TOPOLOGY)
        assert e.value.code == engine.EINVAL
    with pytest.raises(engine.PmlError) as e:                   # not square
        engine.nj_from_matrix(names, m[:, :3])
    assert e.value.code == engine.EINVAL
    import ctypes as C
    L = engine._lib.load()
    na = (C.c_char_p * 4)(*[s.encode() for s in names])
    out = C.c_void_p()
    dp = m.ctypes.data_as(C.POINTER(C.c_double))
    assert L.pml_nj_from_matrix(4, None, dp, 0, 0, C.byref(out)) == engine.EINVAL
    assert L.pml_nj_from_matrix(4, na, None, 0, 0, C.byref(out)) == engine.EINVAL
    assert L.pml_nj_from_matrix(4, na, dp, 0, 0, None) == engine.EINVAL
    assert L.pml_nj_from_matrix(4, na, dp, 2, 0, C.byref(out)) == engine.EINVAL      # neither DISTANCE nor SIMILARITY
    assert L.pml_nj_from_matrix(4, na, dp, 0, 2, C.byref(out)) == engine.EINVAL      # neither form
    assert L.pml_pairscore_table_blosum62(None) == engine.EINVAL


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_golden_cases(case):
    names = case["names"]
    if "rows" in case:
        m = nj_ref.pairwise_scores(case["rows"], FIX["table"])
        assert m == case["scores"]
    else:
        m = case["matrix"]
    for form, key, ref in ((engine.NJ_TREE, "tree", nj_ref.nj_tree_string), (engine.NJ_TOPOLOGY, "topology", nj_ref.nj_topology)):
        same_tree(engine.nj_from_matrix(names, m, case["matrix_type"], form), case[key])
        same_tree(ref(names, m, case["matrix_type"]), case[key])
    lens = [struct.unpack("<d", x)[0] for x in nj_ref.split_tree(case["tree"])[1]]
    if case["name"] == "worked5":
        assert m[0] == [57, 55, 49, 31, 18] and m[4] == [18, 18, 25, 43, 52]
        assert case["tree"] == "(((d:0.0,e:14.166666666666666):17.25,c:1.25):7.0,a:0.5,b:1.5);"
    if case["name"] == "worked4":
        assert case["tree"] == "((c:1.0,d:18.0):7.0,a:0.5,b:1.5);"
    if case["name"] == "q_tie":
        assert case["tree"] == "((a:1.0,b:1.0):0.0,c:1.0,d:1.0);"
    if case["name"] == "identical_rows":
        assert case["rows"][0] == case["rows"][1] and m[0] == m[1]
    if case["name"] == "negative_final_length":
        assert min(lens[-3:]) < 0 and min(lens[:-3]) >= 0
    if case["name"] == "absent_taxon":
        i = names.index("t2")
        assert case["rows"][i].endswith("????") and [g["names"] for g in case["genes"]][1].count("t2") == 0


def test_nj_source_under_host_sanitizers(tmp_path):
    """nj.cpp is plain C++: built alone with a small main under AddressSanitizer and UndefinedBehaviorSanitizer and run as a
    program of its own over seeded random matrices; the sanitizer runtimes are linked statically, so the program needs
    nothing from its environment"""
    exe = str(tmp_path / "nj_standalone")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", os.path.join(ROOT, "pepr_amd", "csrc", "nj.cpp"),
                           os.path.join(ROOT, "tests", "nj_standalone", "main.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "nj_standalone ok: 480 trees, 207 refused bytes" in r.stdout and "ERROR" not in r.stderr
