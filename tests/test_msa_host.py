"""The multiple-alignment rule on the CPU: pml_msa_align_host, pml_msa_profile_align_host and pml_msa_guide_tree_host against
tests/msa_ref.py, exactly -- scores, paths, rows and merges."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from pepr_amd import _lib, engine, tree_builder
import msa_ref as ref
import sw_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
NEW_SYMBOLS = ["pml_msa_align", "pml_msa_align_host", "pml_msa_profile_align", "pml_msa_profile_align_host", "pml_msa_guide_tree_host",
               "pml_msa_result_free", "pml_msa_limits", "pml_debug_msa_profile_align", "pml_msa_stats"]
EINVAL = -1             # PML_EINVAL


def check_profile(X, Y, **opts):
    got = engine.msa_profile_align_host(X, Y, **opts)
    score, path, rows = ref.profile_align(X, Y, opts.get("table"), opts.get("gap_open", 11), opts.get("gap_extend", 1))
    assert got["score"] == score
    assert got["path"] == path
    assert got["rows"] == rows
    assert got["merges"] == [(0, len(X), 1, score)]
    return got


def check_set(seqs, **opts):
    got = engine.msa_align_host([seqs], **opts)[0]
    want = ref.align_set(seqs, opts.get("table"), opts.get("gap_open", 11), opts.get("gap_extend", 1))
    assert got["merges"] == want["merges"]
    assert got["rows"] == want["rows"]
    return got


def test_symbols_and_header():
    header = open(os.path.join(ROOT, "include", "peprml.h")).read()
    L = _lib.load()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, header), s
        assert s in _lib.SYMBOLS, s
        assert hasattr(L, s), s
    for text in ("Multiple alignment", "PARITY WITH muscle IS UNPINNED", "NOT BUILT", "k-mer distances", "Kimura", "bipartitioning", "log-expectation",
                 "anchors and diagonals", "Hirschberg", "128-bit", "Minus\n * infinity is -2^30", ">= 2^30", ":701-725", ":737-806", ":90-141", ":143-218"):
        assert text in header, text
    for doc, text in (("README.md", "parity with muscle is unpinned"), ("DESIGN.md", "Multiple alignment kernels"), ("SURVEY.md", "Since built"),
                      ("INTEGRATION.md", "MultipleSequenceAligner.getMSA")):
        assert text in open(os.path.join(ROOT, doc)).read(), (doc, text)
    lim = engine.msa_limits()
    assert lim["strip"] == 8 and lim["rows"] == [l * 8 for l in lim["lanes"]] and lim["lanes"] == sorted(lim["lanes"])


def test_hand_checked_pairs():
    """BLOSUM62, costs 11 / 1, one row each (w = 1): A-A 4, W-W 11, A-W -3.
    (a) an end gap pays no open cost.  X = AW, Y = W: H[1][0] = F[1][0] = -1 (oF(0) = 0), H[2][1] = H[1][0] + 11 = 10.  With an
        open cost the gap would cost 12 and the score be -1.  Path: X's A alone, then W-W.
    (b) an inner gap pays it.  X = WWAWW, Y = WWWW: four W-W and A against a gap inside Y, 44 - (11 + 1) = 32; the ungapped
        placements (A-W -3 and one end column -1) give 29.
    (c) diagonal before E.  X = A, Y = AA: H[1][2] is 3 both ways: diagonal H[0][1] + 4 = -1 + 4 and E[1][2] = H[1][1] - oE(1) - 1 =
        4 - 0 - 1 (row 1 is X's last: oE = 0).  The diagonal wins: X's A faces Y's LAST A.
    (d) E before F.  X = A, Y = W: diagonal -3; E[1][1] = H[1][0] - 0 - 1 = -2; F[1][1] = H[0][1] - 0 - 1 = -2.  E wins: the walk
        takes Y's column first (going back), so X's column comes first in the alignment.
    (e) open before extend.  X = A, Y = AAW: H[1][1] = 4, E[1][2] = max(E[1][1] - 1 = -3, H[1][1] - 1 = 3) = 3 = H[1][2] (and the
        diagonal -1 + 4 = 3 ties there), E[1][3] = max(E[1][2] - 1, H[1][2] - 0 - 1) = 2 both ways, the diagonal at (1, 3) is
        -2 - 3 = -5, so H[1][3] = 2 from E.  The run OPENS at (1, 3): the walk returns to H at (1, 2), where the diagonal is
        preferred: X's A faces Y's middle A.  Had it extended, it would have stayed in E and put X's A on Y's first A."""
    r = check_profile(["AW"], ["W"])
    assert (r["score"], r["path"], r["rows"]) == (10, [2, 0], ["AW", "-W"])
    r = check_profile(["WWAWW"], ["WWWW"])
    assert (r["score"], r["path"], r["rows"]) == (32, [0, 0, 2, 0, 0], ["WWAWW", "WW-WW"])
    r = check_profile(["A"], ["AA"])
    assert (r["score"], r["path"], r["rows"]) == (3, [1, 0], ["-A", "AA"])
    r = check_profile(["A"], ["W"])
    assert (r["score"], r["path"], r["rows"]) == (-2, [2, 1], ["A-", "-W"])
    r = check_profile(["A"], ["AAW"])
    assert (r["score"], r["path"], r["rows"]) == (2, [1, 0, 1], ["-A-", "AAW"])


def test_guide_tree_ties_exact_averages_and_roles():
    # all scores equal: every tie goes to the lowest first id, then the lowest second id
    S = np.full((5, 5), 7, dtype=np.int64)
    assert engine.msa_guide_tree_host(S) == [(0, 1, 1), (0, 2, 2), (0, 3, 3), (0, 4, 4)] == ref.guide_tree(S.tolist())
    # balanced: (0, 1) and (2, 3) first, both at level 1, then the two clusters at level 2
    S = np.zeros((4, 4), dtype=np.int64)
    S[0, 1], S[2, 3] = 50, 40
    assert engine.msa_guide_tree_host(S) == [(0, 1, 1), (2, 3, 1), (0, 2, 2)] == ref.guide_tree(S.tolist())
    # only the exact comparison orders these: after (0, 1) the average of {0, 1} x {2} is (2^62 + 1) / 2 = 2^61 + 1/2 and S(3, 4) is
    # 2^61 + 1.  In doubles both round to 2^61, a tie that would go to (0, 2); exactly, (3, 4) is larger.
    S = np.zeros((5, 5), dtype=np.int64)
    S[0, 1], S[0, 2], S[1, 2], S[3, 4] = 2 ** 62, 2 ** 61, 2 ** 61 + 1, 2 ** 61 + 1
    assert float(2 ** 62 + 1) / 2 == float(2 ** 61 + 1)
    assert engine.msa_guide_tree_host(S) == [(0, 1, 1), (3, 4, 1), (0, 2, 2), (0, 3, 3)] == ref.guide_tree(S.tolist())
    # sums of 2^57 times cluster sizes of up to 16 leave 64 bits
    rng = np.random.default_rng(3)
    for n in (2, 3, 8, 9):
        S = (2 ** 56 + rng.integers(0, 8, (n, n))).astype(np.int64)
        assert engine.msa_guide_tree_host(S) == ref.guide_tree(S.tolist())
    # the lower id is X: its rows come first in the merge, the final rows are back in input order
    a, b = "MKVLAAGIWDERT", "MKVLGGIWDERT"
    got = check_set(["PPPPPPP", a, b])
    assert got["merges"][0][:3] == (1, 2, 1) and got["merges"][1][:3] == (0, 1, 2)
    assert [ref.degap(r) for r in got["rows"]] == ["PPPPPPP", a, b]


@pytest.mark.parametrize("nX,nY", [(1, 1), (1, 2), (2, 1), (2, 5), (5, 2), (5, 5), (1, 5)])
def test_profile_alignment_random_and_planted(nX, nY):
    rng = np.random.default_rng(100 * nX + nY)
    mild, wild = ref.asym_tables()
    X, Y = ref.random_profile(rng, nX, 23), ref.random_profile(rng, nY, 17)
    check_profile(X, Y)
    check_profile(Y, X)
    check_profile(X, Y, gap_open=3, gap_extend=2)
    for t in (mild, wild, mild.T.copy(), wild.T.copy()):
        check_profile(X, Y, table=t)
        check_profile(Y, X, table=t)
    edge = np.full((24, 24), -127, dtype=np.int64)
    edge[np.diag_indices(24)] = 127
    check_profile(X, Y, table=edge)
    # planted: the two halves of a family with deletions, aligned among themselves first
    fam = ref.family(rng, nX + nY, 40, deletions=1, truncate=True)
    A = engine.msa_align_host([fam[:nX]])[0]["rows"]
    B = engine.msa_align_host([fam[nX:]])[0]["rows"]
    check_profile(A, B)


def test_int32_bound_just_under_and_just_over():
    rng = np.random.default_rng(8)
    X, Y = ref.random_profile(rng, 5, 45, 0.1), ref.random_profile(rng, 5, 43, 0.1)
    table = sw_ref.blosum62()
    go = max(g for g in range(2 ** 19, 2 ** 20) if ref.bound(5, 5, 45, 43, table, g, 1) < 2 ** 30)
    assert ref.bound(5, 5, 45, 43, table, go + 1, 1) >= 2 ** 30 and go + 1 <= 2 ** 20
    check_profile(X, Y, gap_open=go)
    with pytest.raises(engine.PmlError) as e:
        engine.msa_profile_align_host(X, Y, gap_open=go + 1)
    assert e.value.code == EINVAL and "set 0" in str(e.value) and "2^30" in str(e.value)
    # a whole set: the last merges of twelve sequences of 300 residues pass the bound at the largest open cost; the set is named
    fam = ref.family(rng, 12, 300)
    with pytest.raises(engine.PmlError) as e:
        engine.msa_align_host([["ACDE", "ACDF"], fam], gap_open=2 ** 20)
    assert e.value.code == EINVAL and "set 1" in str(e.value) and "2^30" in str(e.value)


def test_properties_on_random_sets():
    rng = np.random.default_rng(21)
    sets = []
    for n in (1, 2, 3, 5, 8):
        sets.append(ref.family(rng, n, int(rng.integers(20, 50)), deletions=1, truncate=n >= 3, alphabet=sw_ref.ALPHABET))
    sets.append([sw_ref.random_protein(rng, int(k)) for k in rng.integers(1, 30, 6)])          # unrelated, lengths from 1
    res = engine.msa_align_host(sets)
    for seqs, r in zip(sets, res):
        rows = r["rows"]
        assert len(rows) == len(seqs) and len({len(x) for x in rows}) == 1
        assert [ref.degap(x) for x in rows] == [ref.clean(s) for s in seqs]
        assert not any(all(x[c] == "-" for x in rows) for c in range(len(rows[0])))
        assert len(r["merges"]) == len(seqs) - 1
    assert res[0]["rows"] == [ref.clean(sets[0][0])]
    for seqs in sets[1:4] + sets[5:]:
        check_set(seqs)
    # substitutions only: no gap anywhere
    fam = ref.family(rng, 6, 70, frac=0.1)
    assert check_set(fam)["rows"] == fam
    # planted deletions come back as gaps of the planted length
    root = sw_ref.random_protein(rng, 70, ref.PLAIN)
    cut = root[:30] + root[34:]
    got = check_set([root, cut, sw_ref.mutate(rng, root), sw_ref.mutate(rng, cut)])
    assert got["rows"][1].count("-") == 4 and got["rows"][3].count("-") == 4 and "-" not in got["rows"][0] + got["rows"][2]


def test_other_costs_and_asymmetric_tables_on_sets():
    rng = np.random.default_rng(5)
    mild, wild = ref.asym_tables()
    fam = ref.family(rng, 5, 30, deletions=1)
    check_set(fam, gap_open=3, gap_extend=2)
    check_set(fam, table=mild)
    check_set(fam, table=wild)
    check_set(fam[::-1], table=wild)


def test_invalid_input():
    for bad, text in (([["ACD", ""]], "set 0, sequence 1 is empty"), ([["ACD"], ["AC-D"]], "set 1, sequence 0"), ([["A1"]], "position 1")):
        with pytest.raises(engine.PmlError) as e:
            engine.msa_align_host(bad)
        assert e.value.code == EINVAL and text in str(e.value), str(e.value)
    t = sw_ref.blosum62().copy()
    t[3][4] = 128
    with pytest.raises(engine.PmlError) as e:
        engine.msa_align_host([["ACD", "ACD"]], table=t)
    assert "int8" in str(e.value)
    with pytest.raises(engine.PmlError) as e:
        engine.msa_profile_align_host(["ACD", "AC"], ["ACD"])
    assert "columns" in str(e.value)


def test_host_half_standalone_under_host_sanitizers(tmp_path):
    """msa_host.cpp is plain C++: built ALONE (with sw_host.cpp and nj.cpp) and a small main under AddressSanitizer and
    UndefinedBehaviorSanitizer and run as a program of its own on a few sets and a profile pair; its output equals the reference"""
    exe = str(tmp_path / "msa_standalone")
    src = os.path.join(ROOT, "pepr_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", os.path.join(src, "msa_host.cpp"), os.path.join(src, "sw_host.cpp"), os.path.join(src, "nj.cpp"),
                           os.path.join(ROOT, "tests", "msa_standalone", "main.cpp"), "-o", exe])
    rng = np.random.default_rng(17)
    sets = [ref.family(rng, 4, 25, deletions=1, truncate=True), [sw_ref.random_protein(rng, 9)], ref.family(rng, 3, 12, alphabet=sw_ref.ALPHABET)]
    X, Y = ref.random_profile(rng, 2, 11), ref.random_profile(rng, 3, 8)
    text = "".join("S\n" + "".join("Q %s\n" % s for s in st) for st in sets) + "".join("P\n" + "".join("Q %s\n" % s for s in p) for p in (X, Y))
    out = subprocess.run([exe, "3", "2"], input=text.encode(), capture_output=True, timeout=120)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    want = ["rc 0 "]
    for k, st in enumerate(sets):
        r = ref.align_set(st, None, 3, 2)
        want += ["set %d" % k] + ["row " + x for x in r["rows"]] + ["merge %d %d %d %d" % m for m in r["merges"]]
    score, path, rows = ref.profile_align(X, Y, None, 3, 2)
    want += ["profile rc 0 score %d" % score] + ["row " + x for x in rows] + ["merge 0 %d 1 %d" % (len(X), score), "path " + "".join(str(p) for p in path)]
    assert out.stdout.decode().split("\n")[:-1] == want
    bad = subprocess.run([exe], input=b"S\nQ ACD\nQ\n", capture_output=True, timeout=120)
    assert bad.returncode == 0 and bad.stdout.decode().startswith("rc -1 set 0, sequence 1 is empty"), bad.stdout.decode() + bad.stderr.decode()[-2000:]


def test_mirror_class_and_tool_through_the_host_twin(tmp_path):
    import pepr_align_sets
    import pepr_tree_step
    rng = np.random.default_rng(4)
    genomes = sw_ref.planted_families(seed=9, ngenomes=4, nfam=2, length=40)
    gfiles = []
    for g, genome in enumerate(genomes):
        p = str(tmp_path / ("genome%d.faa" % g))
        with open(p, "w") as fh:
            for title, res in genome:
                fh.write(">%s\n%s\n" % (title, res))
        gfiles.append(p)
    hg = tmp_path / "hg_run"
    hg.mkdir()
    set_files = []
    for f in range(2):
        p = str(hg / ("set_%d.faa" % f))
        with open(p, "w") as fh:
            for genome in genomes:
                fh.write(">%s\n%s\n" % genome[f])
        set_files.append(p)
    out = str(tmp_path / "aligned")
    assert pepr_align_sets.main(["-sets"] + set_files + ["-genome_file"] + gfiles + ["-o", out, "-host", "true"]) == 0
    for f in range(2):
        names, rows = pepr_tree_step.read_fasta(os.path.join(out, "set_%d_align.faa" % f))
        assert names == ["genome_%d" % g for g in range(4)]
        assert rows == ref.align_set([genome[f][1] for genome in genomes])["rows"]
    aligner = tree_builder.MultipleSequenceAligner(host=True)
    a = aligner.getMSA(tree_builder.SequenceAlignment(["t0", "t1", "t2"], ref.family(rng, 3, 30, deletions=1), "set_7"))
    assert a.getName() == "set_7_align" and a.getTaxa() == ["t0", "t1", "t2"] and len({len(r) for r in a.rows}) == 1
    b = aligner.getMSA([("u0", "ACDEFGHIK"), ("u1", "ACDFGHIK")])
    assert b.getName() == "null_align" and b.rows == ["ACDEFGHIK", "ACD-FGHIK"]
    p = aligner.getProfileMSA(a, b)
    assert p.getTaxa() == ["t0", "t1", "t2", "u0", "u1"] and p.getName() == "set_7_align_align"
    assert p.rows == ref.profile_align(a.rows, b.rows)[2]
    many = aligner.getMSAs([[("x", "ACD")], [("y", "WWW"), ("z", "WW")]], names=["s0", "s1"])
    assert [m.getName() for m in many] == ["s0_align", "s1_align"] and many[0].rows == ["ACD"]
