"""The host half of the MinHash path (no GPU): the host doors of the rule and of the Java's selection routines against the
restatement (mash_ref.py), the two hash restatements against each other, mash_host.cpp alone under host sanitizers as a program
of its own, and the NeighborMasher mirror and tool with the device call stubbed out."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from pepr_amd import _lib, engine, tree_builder
import mash_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import pepr_neighbor_masher  # noqa: E402

GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "mash_cases.json")))
KS = (1, 8, 9, 15, 16, 17, 21, 31, 32)
NEW_SYMBOLS = ["pml_mash_tile", "pml_mash_chunk", "pml_mash_sketch", "pml_mash_dist", "pml_mash_distances", "pml_debug_mash_hashes", "pml_debug_mash_full_sort",
               "pml_mash_stats", "pml_mash_murmur3", "pml_mash_hashes_host", "pml_mash_sketch_host", "pml_mash_pair_host", "pml_mash_distance_of",
               "pml_mash_candidate_distances", "pml_mash_expand_ingroup", "pml_mash_pair_stats", "pml_mash_select_outgroup", "pml_neighbor_masher",
               "pml_neighbor_masher_result_free"]
BASES = np.frombuffer(b"ACGT", dtype=np.uint8)


def odd_genome(rng, k):
    """records around k, lower case, other bytes, an empty record"""
    noisy = BASES[rng.integers(0, 4, 400)].copy()
    noisy[rng.integers(0, 400, 12)] = np.frombuffer(b"NnRY-\x00\xff@[`{U", dtype=np.uint8)
    low = BASES[rng.integers(0, 4, 120)].tobytes().lower()
    return [BASES[rng.integers(0, 4, n)].tobytes() for n in (max(k - 1, 0), k, k + 1, 3 * k + 2)] + [noisy.tobytes(), b"", low, b"ACGT" * 12, b"GAATTC" * 7]


def same_float(a, b):
    return a == b or (a != a and b != b)


def within_2ulp(a, b):
    return abs(a - b) <= 2 * np.spacing(max(abs(a), abs(b)))


def test_new_symbols_are_declared_listed_and_exported():
    header = open(os.path.join(ROOT, "include", "peprml.h")).read()
    L = _lib.load()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, header), s
        assert s in _lib.SYMBOLS, s
        assert hasattr(L, s), s
    for text in ("PARITY WITH THE mash BINARY IS UNPINNED", "Ondov et al. 2016", "0x87c37b91114253d5", "b4e9c495b633d387", "util/NeighborMasher.java",
                 ":281-324", ":738-783", ":483-568", ":855-867", "input order", "six significant digits", "UNROOTED"):
        assert text in header, text
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert re.search(r"parity with the mash binary is unpinned", open(os.path.join(ROOT, doc)).read(), re.I), doc
    assert engine.mash_tile() >= 64 and engine.mash_chunk() >= 64


def test_hash_vectors_and_the_two_restatements():
    for v in GOLD["hash_vectors"]:
        data = v["text"].encode()
        h = ref.murmur3_x64_128(data, v["seed"])
        assert "%016x" % h[0] == v["h1"] and (v["h2"] is None or "%016x" % h[1] == v["h2"])
        assert engine.mash_murmur3(data, v["seed"]) == h
    rng = np.random.default_rng(1)
    for n in list(range(0, 50)) + [63, 64, 65, 200]:
        rows = rng.integers(0, 256, (7, n), dtype=np.uint8)
        vec = ref.murmur_h1_rows(rows, 42) if n else None
        for i in range(7):
            h = ref.murmur3_x64_128(rows[i].tobytes(), 42)
            assert engine.mash_murmur3(rows[i].tobytes(), 42) == h
            if n:
                assert int(vec[i]) == h[0], (n, i)


@pytest.mark.parametrize("k", KS)
def test_host_values_and_sketches_equal_the_restatement(k):
    rng = np.random.default_rng(10 + k)
    g = odd_genome(rng, k)
    got = engine.mash_hashes_host(g, k)
    slow = np.array([v for r in g for v in ref.record_values_slow(r, k)], dtype=np.uint64)
    assert (got == slow).all() and (ref.hashes(g, k) == slow).all()
    if k <= 16:
        assert int(got[got != ref.INVALID].max()) < 1 << 32
    D = np.unique(slow[slow != ref.INVALID]).size
    for s in (1, 7, D - 1, D, D + 1, 100000):
        if s < 1:
            continue
        sk = engine.mash_sketch_host(g, k, s)
        assert sk.size == min(s, D) and (sk == ref.sketch(g, k, s)).all()
    assert engine.mash_sketch_host([b"", b"ACG"[:max(k - 1, 0)], b"NNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNN"], k, 5).size == 0
    assert engine.mash_sketch_host([], k, 5).size == 0


def test_canonical_4mers_and_palindromes():
    import itertools
    recs = ["".join(p) for p in itertools.product("ACGT", repeat=4)]
    assert engine.mash_sketch_host(recs, 4, 1000).size == GOLD["canonical_4mers"]["distinct"]
    one = "".join(recs)
    assert engine.mash_sketch_host([one + one[:3]], 4, 1000).size <= 136
    assert ref.window_value(b"ACGT", 4) == ref.murmur3_x64_128(b"ACGT", 42)[0] & 0xFFFFFFFF          # its own reverse complement
    assert ref.window_value(b"TTTT", 4) == ref.window_value(b"aaaa", 4) == ref.murmur3_x64_128(b"AAAA", 42)[0] & 0xFFFFFFFF
    assert ref.window_value(b"ACGN", 4) is None


def test_refusals_of_the_host_doors():
    for k, s in ((0, 5), (33, 5), (21, 0), (-1, 5)):
        with pytest.raises(engine.PmlError) as e:
            engine.mash_sketch_host([b"ACGT" * 20], k, s)
        assert e.value.code == engine.EINVAL
    with pytest.raises(engine.PmlError):
        engine.mash_hashes_host([b"ACGT"], 40)
    with pytest.raises(engine.PmlError):
        engine.mash_pair_host([1], [2], 0)


def test_pairs_golden_and_random_against_the_loop():
    for case in GOLD["pairs"]:
        assert engine.mash_pair_host(case["a"], case["b"], case["s"]) == (case["common"], case["denom"]) == ref.pair(case["a"], case["b"], case["s"]), case["name"]
        if "distance" in case:
            assert engine.mash_distance_of(case["common"], case["denom"], 21) == case["distance"] == ref.distance(case["common"], case["denom"], 21)
    rng = np.random.default_rng(2)
    universe = np.unique(rng.integers(0, 1 << 63, 400, dtype=np.uint64))
    for _ in range(60):
        a = np.sort(rng.choice(universe, rng.integers(0, 200), replace=False))
        b = np.sort(rng.choice(universe, rng.integers(0, 200), replace=False))
        for s in (1, 5, 150, 199, 200, 500):
            want = ref.pair(a[:s], b[:s], s)
            assert engine.mash_pair_host(a[:s], b[:s], s) == want == ref.pair_fast(a[:s], b[:s], s)


def test_distances_special_values_exact_and_the_rest_within_2_ulp():
    for k in KS:
        for denom in (1, 2, 7, 200, 100000):
            assert engine.mash_distance_of(denom, denom, k) == 0.0 and engine.mash_distance_of(0, denom, k) == 1.0
            for common in sorted({1, denom // 3, denom // 2, denom - 1} - {0, denom}):
                got, want = engine.mash_distance_of(common, denom, k), ref.distance(common, denom, k)
                assert within_2ulp(got, want) and 0.0 < got <= 1.0
                d6 = engine.mash_distance_of(common, denom, k, 6)
                assert d6 == float("%.6g" % got) and within_2ulp(d6, ref.distance(common, denom, k, 6))
    assert engine.mash_distance_of(0, 0, 21) == 0.0                                      # two empty sketches, by the rule
    assert engine.mash_distance_of(1, 100000, 1) == 1.0                                  # the cap


def random_table(rng, n_pool, n_in):
    """distances on a coarse grid, so that ties are many, with entries of exactly 1.0"""
    d = rng.integers(1, 12, (n_pool, n_in)) / 16.0
    d[rng.random((n_pool, n_in)) < 0.1] = 1.0
    return d


def test_selection_routines_on_random_tables_with_ties():
    rng = np.random.default_rng(3)
    for trial in range(200):
        n_in, n_pool = int(rng.integers(1, 6)), int(rng.integers(0, 14))
        d = random_table(rng, n_pool, n_in)
        flags = [bool(x) for x in rng.random(n_pool) < 0.2]
        cand = engine.mash_candidate_distances(d) if n_pool else np.zeros(0)
        assert list(cand) == ref.candidate_distances(d.tolist()) == [ref.distance_from_ingroup(r) for r in d.tolist()]
        for target in (0, n_in, n_in + 1, n_in + 3, 40):
            assert engine.mash_expand_ingroup(d, target, flags) == ref.expand_ingroup(d.tolist(), flags, target), (trial, target)
        assert engine.mash_expand_ingroup(d, n_in + 2) == ref.expand_ingroup(d.tolist(), [False] * n_pool, n_in + 2)
        dff = rng.integers(1, 8, (n_in, n_in)) / 16.0
        pd = ref.ingroup_pair_distances(dff.tolist())
        mean, sd, mx = engine.mash_pair_stats(pd)
        wmean = ref.get_mean(pd)
        assert same_float(mean, wmean) and same_float(sd, ref.get_standard_deviation(pd, wmean)) and same_float(mx, ref.get_max(pd))
        for count in (0, 1, 2, 3, 5):
            for m, dev in ((mx, sd), (0.25, 0.0), (0.0, 0.1), (2.0, 0.0)):
                assert engine.mash_select_outgroup(cand, m, dev, count) == ref.select_outgroup(list(cand), m, dev, count), (trial, count, m, dev)


def test_selection_single_pair_single_taxon_and_golden():
    mean, sd, mx = engine.mash_pair_stats([0.125])                                       # one ingroup pair: sd is 0 / 0
    assert mean == 0.125 and sd != sd and mx == 0.125
    cand = [0.5, 0.25, 0.0625, 1.0]
    assert engine.mash_select_outgroup(cand, mx, sd, 3) == ref.select_outgroup(cand, mx, sd, 3) == [0]       # NaN threshold: all too near, the farthest one
    mean, sd, mx = engine.mash_pair_stats([])                                            # one ingroup taxon: no pair
    assert mean != mean and mx != mx and sd == 0.0 and np.signbit(sd)
    assert engine.mash_select_outgroup(cand, mx, sd, 3) == ref.select_outgroup(cand, mx, sd, 3) == [0]
    assert engine.mash_select_outgroup([1.0, 1.0], 0.1, 0.0, 3) == []                    # only too-far candidates
    for case in GOLD["selection"]:
        assert engine.mash_select_outgroup(case["cand"], case["max_ingroup"], case["sd"], case["count"]) == case["selected"] == \
            ref.select_outgroup(case["cand"], case["max_ingroup"], case["sd"], case["count"]), case["name"]
    assert engine.mash_pair_stats([0.5, float("nan"), 0.25])[0] == 0.375                # getMean skips NaN


def hexrec(r):
    return r.hex() if r else "-"


def test_host_half_standalone_under_host_sanitizers(tmp_path):
    """mash_host.cpp is plain C++: built ALONE with a small main under AddressSanitizer and UndefinedBehaviorSanitizer and run as a
    program of its own on valid, odd and mutated inputs; its values equal the restatement's"""
    exe = str(tmp_path / "mash_standalone")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", os.path.join(ROOT, "pepr_amd", "csrc", "mash_host.cpp"),
                           os.path.join(ROOT, "tests", "mash_standalone", "main.cpp"), "-o", exe])
    rng = np.random.default_rng(4)
    lines, checks = [], []
    for k in KS:
        g = odd_genome(rng, k)
        mutated = [bytes(rng.integers(0, 256, len(r), dtype=np.uint8)) if i % 2 else r for i, r in enumerate(g)]
        for genome, s in ((g, 50), (mutated, 3), ([], 5), ([b""], 1)):
            lines += ["G %d %d %d" % (k, s, len(genome))] + [hexrec(r) for r in genome]
            checks.append(("G", genome, k, s))
    universe = np.unique(rng.integers(0, 1 << 64, 300, dtype=np.uint64))
    for na, nb, s in ((0, 0, 4), (0, 9, 4), (50, 70, 60), (120, 120, 100), (5, 200, 1), (200, 200, 1000)):
        a, b = np.sort(rng.choice(universe, na, replace=False)), np.sort(rng.choice(universe, nb, replace=False))
        lines += ["P 21 %d %d %d" % (s, na, nb), " ".join(map(str, a)) or "-", " ".join(map(str, b)) or "-"]
        checks.append(("P", a, b, s))
    for n in (0, 1, 2, 6):
        d = (rng.integers(1, 9, n) / 16.0).tolist()
        lines += ["T %d" % n, " ".join(repr(x) for x in d)]
        checks.append(("T", d))
    for n_in, n_pool, target in ((1, 0, 3), (2, 5, 4), (3, 9, 20), (4, 6, 4)):
        d = random_table(rng, n_pool, n_in)
        flags = [int(x) for x in rng.random(n_pool) < 0.3]
        lines += ["E %d %d %d" % (n_in, n_pool, target)] + [" ".join(repr(x) for x in row) for row in d.tolist()] + [" ".join(map(str, flags)) or "-"]
        checks.append(("E", d.tolist(), flags, target))
        cand = ref.candidate_distances(d.tolist())
        for mx, sd, count in ((0.25, 0.0, 2), (float("nan"), float("nan"), 3), (0.0, 0.5, 0), (0.1, 0.1, 9)):
            lines += ["S %d %d %r %r" % (n_pool, count, mx, sd), " ".join(repr(x) for x in cand)]
            checks.append(("S", cand, mx, sd, count))
    lines += ["G 0 5 1", "41", "G 33 5 1", "41", "G 21 0 1", "41", "P 21 0 1 1", "1", "2"]                  # refusals come back as error lines
    path = str(tmp_path / "cases.txt")
    open(path, "w").write("\n".join(lines) + "\n")
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stdout[-1000:], r.stderr[-3000:])
    out = iter(r.stdout.splitlines())
    for c in checks:
        if c[0] == "G":
            _, genome, k, s = c
            vals = next(out).split()[1:]
            assert [int(x, 16) for x in vals] == [int(x) for x in ref.hashes(genome, k)]
            assert [int(x, 16) for x in next(out).split()[1:]] == [int(x) for x in ref.sketch(genome, k, s)]
        elif c[0] == "P":
            f = next(out).split()
            common, denom = ref.pair(c[1], c[2], c[3])
            assert (int(f[1]), int(f[2])) == (common, denom)
            assert within_2ulp(float.fromhex(f[3]), ref.distance(common, denom, 21)) and within_2ulp(float.fromhex(f[4]), ref.distance(common, denom, 21, 6))
        elif c[0] == "T":
            f = next(out).split()
            mean = ref.get_mean(c[1])
            for got, want in zip(f[1:], (mean, ref.get_standard_deviation(c[1], mean), ref.get_max(c[1]))):
                assert same_float(float.fromhex(got), want) if "nan" not in got else want != want
        elif c[0] == "E":
            assert [int(x) for x in next(out).split()[1:]] == ref.expand_ingroup(c[1], c[2], c[3])
            assert [float.fromhex(x) for x in next(out).split()[1:]] == ref.candidate_distances(c[1])
        else:
            assert [int(x) for x in next(out).split()[1:]] == ref.select_outgroup(c[1], c[2], c[3], c[4])
    assert list(out) == ["error -1"] * 4


class StubContext:
    """stands in for engine.Context: records the call and answers with a canned result"""

    def __init__(self):
        self.calls = []

    def neighbor_masher(self, ingroup, pool, **kw):
        self.calls.append((ingroup, pool, kw))
        return {"ingroup": [t[0] for t in ingroup], "outgroup": [t[0] for t in pool[:1]], "taxa": [], "ingroup_tree": "(a,b,(c,d));" if kw["expand_ingroup"] > 3 else None,
                "rooted_tree": "(o,a,(b,(c,d)));" if not kw["ingroup_only"] else None}


def test_neighbor_masher_mirror_passes_the_javas_settings():
    ctx = StubContext()
    nm = tree_builder.NeighborMasher(ctx)
    nm.setIngroupGenomes([("a", [b"ACGT"])]); nm.setOutgroupGenomes([("o", [b"ACGA"])])
    nm.run()
    assert ctx.calls[0][2] == dict(k=21, s=100000, outgroup_count=3, expand_ingroup=0, ingroup_only=False, outgroup_only=False, digits=6)      # :45-57
    nm.setMashKmerLength(15); nm.setMashSketchSize(500); nm.setOutgroupCount(2); nm.setExpandedIngroupSize(8); nm.setIngroupTreeOnly(True)
    nm.setOutgroupOnly(True); nm.setDistanceDigits(None); nm.setRunName("r")
    nm.run()
    assert ctx.calls[1][2] == dict(k=15, s=500, outgroup_count=2, expand_ingroup=8, ingroup_only=True, outgroup_only=True, digits=None)
    assert nm.getRunName() == "r" and nm.getIngroupTaxa() == ["a"] and nm.getSelectedOutgroupTaxa() == ["o"] and nm.getIngroupTree() == "(a,b,(c,d));"
    assert nm.getRootedTree() is None


def test_taxon_from_title_restatements_agree():
    for title, want in ((">NC_000913.3 Escherichia coli [Escherichia coli str. K-12 | 511145.12]", "Escherichia_coli_str._K-12_@_511145.12"),
                        (">plain title, no brackets", "plain_title_no_brackets"), ("no marker (x):y", "no_marker_x_y"),
                        (">a [b [c] d] e", "b_c_d"), ("]>odd", "]>odd".replace("]", "_")), (">x [y]|z [w|v]", "w@v"), (">a  b", "a_b"), (">a   b", "a_b")):
        got = pepr_neighbor_masher.taxon_from_title(title)
        assert got == ref.taxon_from_title(title), title
        if want is not None:
            assert got == want, (title, got)
    assert pepr_neighbor_masher.id_of("genus_species_@_12.3") == "12.3" and pepr_neighbor_masher.id_of("noid") == "noid"


def test_tool_argument_handling_with_the_device_call_stubbed(tmp_path, capsys, monkeypatch):
    def fasta(name, title, seqs):
        p = str(tmp_path / name)
        open(p, "w").write("".join(">%s\n%s\n" % (title if i == 0 else "rec%d" % i, "\n".join(s[j:j + 10] for j in range(0, len(s), 10))) for i, s in enumerate(seqs)))
        return p
    a = fasta("a.fna", "acc [Genus one | 1.1]", ["ACGTACGTACGTAAC", "", "GGGTTT"])
    b = fasta("b.fna", "acc [Genus two | 2.2]", ["ACGTACGTACGTAAG"])
    o = fasta("o.fna", "acc [Other | 9.9]", ["TTGTACGTACGTAAG"])
    assert pepr_neighbor_masher.read_genome(a) == ("Genus_one_@_1.1", [b"ACGTACGTACGTAAC", b"", b"GGGTTT"])
    ctx = StubContext()
    monkeypatch.chdir(tmp_path)
    run = str(tmp_path / "run1")
    pepr_neighbor_masher.main(["-ingroup", a, b, "-outgroup", o, "-k", "11", "-s", "77", "-outgroup_count", "1", "-expand_ingroup", "5", "-run_name", run,
                               "-mash", "/opt/mash", "-p", "8", "-outgroup_sketch", "x.msh", "-auto_adjust", "true"], ctx=ctx)
    ingroup, pool, kw = ctx.calls[0]
    assert [t[0] for t in ingroup] == ["Genus_one_@_1.1", "Genus_two_@_2.2"] and [t[0] for t in pool] == ["Other_@_9.9"]
    assert kw == dict(k=11, s=77, outgroup_count=1, expand_ingroup=5, ingroup_only=False, outgroup_only=False, digits=6)
    err = capsys.readouterr().err
    for key in ("mash", "p", "outgroup_sketch", "auto_adjust"):
        assert "-%s is ignored" % key in err
    assert open(run + "_ingroup.txt").read() == "1.1\n2.2\n" and open(run + "_outgroup.txt").read() == "9.9\n"
    assert open(run + "_k11_s77_ingroup_nj.nwk").read() == "(a,b,(c,d));" and open(run + "_k11_s77_rooted_nj.nwk").read() == "(o,a,(b,(c,d)));"
    ctx2 = StubContext()
    run2 = str(tmp_path / "run2")
    pepr_neighbor_masher.main(["-ingroup", a, b, "-ingroup_only", "-outgroup_only", "true", "-run_name", run2, "-digits", "0"], ctx=ctx2)
    assert ctx2.calls[0][2] == dict(k=21, s=100000, outgroup_count=3, expand_ingroup=0, ingroup_only=True, outgroup_only=True, digits=0)
    assert os.path.exists(run2 + "_ingroup.txt") and not os.path.exists(run2 + "_outgroup.txt") and not os.path.exists(run2 + "_k21_s100000_ingroup_nj.nwk")
    with pytest.raises(SystemExit):
        pepr_neighbor_masher.main(["-outgroup", o], ctx=StubContext())
