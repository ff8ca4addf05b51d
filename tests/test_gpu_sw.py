"""The homology search on the device (csrc/sw.hip) against the host twin and tests/sw_ref.py, exactly: every class through the test
door at its strip, group and pass boundaries, the stream's resets, ties across chunks and units, a mixed set, the counters
and the whole step from genome files to set files."""
import os
import sys

import numpy as np
import pytest

from pepr_amd import engine, tree_builder
import sw_ref as ref
from sw_ref import PLAIN, mutate, planted_families, random_protein

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIM = engine.sw_class_limits()
T = LIM["strip"]
BATCH = 64                       # stream positions the kernel stages at a time (and reads of the line buffer)


def ref_scores(queries, subjects, **opts):
    return np.asarray([[ref.score(q, s, **opts) for s in subjects] for q in queries], dtype=np.int32)


def gap_subjects(p, at, flank=12):
    """pieces of p around row `at` with three residues cut out (the query's rows at - 1 .. at + 1 face a gap: F crosses the
    boundary) and with three put in (E)"""
    lo, hi = max(at - flank, 0), min(at + flank, len(p))
    cut = p[lo:max(at - 1, lo)] + p[min(at + 2, hi):hi]
    put = p[lo:at] + "WCW" + p[at:hi]
    return [cut, put]


@pytest.mark.parametrize("cls", [0, 1, 2])
def test_debug_scores_at_the_boundaries(gpu_ctx, cls):
    L, rows = LIM["lanes"][cls], LIM["rows"][cls]
    assert rows == L * T
    rng = np.random.default_rng(40 + cls)
    lens = [1, T - 1, T, T + 1, rows - 1, rows] + ([rows + 1, 2 * rows + 1, 2 * rows + 40] if cls == 2 else [])
    queries = [random_protein(rng, n) for n in lens[:-1]] + [random_protein(rng, lens[-1], PLAIN)]
    long_q = queries[-1]
    subjects = [random_protein(rng, n) for n in (1, 2, BATCH + 1)] + [mutate(rng, long_q[: 3 * T].upper())]
    subjects += gap_subjects(long_q, T) + gap_subjects(long_q, 5 * T)
    if cls == 2:
        subjects += gap_subjects(long_q, rows) + gap_subjects(long_q, 2 * rows)       # the pass boundaries
    want = ref_scores(queries, subjects)
    got = gpu_ctx.debug_sw_scores(queries, subjects, force_class=cls)
    print("class", cls, "max |device - ref| =", int(np.abs(got - want).max()))
    assert (got == want).all(), np.argwhere(got != want)[:8]
    for k in range(6, len(subjects)):                                                 # the planted gaps are taken
        assert want[-1, k] > ref.score(long_q, subjects[k], gap_open=1000), k
    other = dict(gap_open=3, gap_extend=2)
    assert (gpu_ctx.debug_sw_scores(queries[2:5], subjects[2:6], force_class=cls, **other) == ref_scores(queries[2:5], subjects[2:6], **other)).all()
    if cls < 2:                                                                       # a class cannot hold a longer query
        with pytest.raises(engine.PmlError) as e:
            gpu_ctx.debug_sw_scores([random_protein(rng, rows + 1)], subjects[:2], force_class=cls)
        assert e.value.code == engine.EINVAL
    with pytest.raises(engine.PmlError) as e:
        gpu_ctx.debug_sw_scores(queries[:1], subjects[:1], force_class=cls, force_path=1)     # no 16-bit path is built
    assert e.value.code == engine.EINVAL


@pytest.mark.parametrize("cls,qlen", [(0, 100), (2, 100), (2, 600)])
def test_streaming_resets(gpu_ctx, cls, qlen):
    rng = np.random.default_rng(7)
    q = random_protein(rng, qlen, PLAIN)
    shorts = [random_protein(rng, 1 + (i & 1), PLAIN) for i in range(40)]
    long_s = mutate(rng, q[:90], 0.1) + random_protein(rng, 60, PLAIN)
    alone = {s: ref.score(q, s) for s in set(shorts + [long_s])}                      # every subject scored alone
    for subjects in (shorts + [long_s], [long_s] + shorts, shorts[:20] + [long_s] + shorts[20:]):
        got = gpu_ctx.debug_sw_scores([q], subjects, force_class=cls)
        assert got[0].tolist() == [alone[s] for s in subjects]
    assert int(gpu_ctx.debug_sw_scores([q], [long_s], force_class=cls)[0, 0]) == alone[long_s] > 150


def test_ties_across_chunks_and_units(gpu_ctx, monkeypatch):
    rng = np.random.default_rng(21)
    p = random_protein(rng, 15, PLAIN)
    fill = lambda n: random_protein(rng, n, "GS")       # noqa: E731
    target = [("t%d" % i, s) for i, s in enumerate([fill(9), p + "PPP", fill(30), fill(12), p, fill(20), fill(5), p, fill(33), fill(14), fill(8), fill(3),
                                                    p, fill(17), fill(26), "GG" + p, fill(11)])]
    queries = [("q%d" % i, s) for i, s in enumerate([p, fill(10), p.lower(), fill(200), p + fill(300)])]
    genomes = [target, queries]
    host = engine.sw_search_host(genomes)
    assert (len(target) + 0, 1) in set(zip(host["query"], host["subject"]))           # five subjects tie at p's self score: position 1 wins
    plain = gpu_ctx.sw_search(genomes)
    monkeypatch.setenv("PML_SW_TINY_UNITS", "1")
    before = gpu_ctx.sw_stats()["units"]
    tiny = gpu_ctx.sw_search(genomes)
    assert gpu_ctx.sw_stats()["units"] - before > 12                                   # the tie's subjects lie in several chunks and units
    monkeypatch.delenv("PML_SW_TINY_UNITS")
    again = gpu_ctx.sw_search(genomes)
    assert plain["table"] == tiny["table"] == again["table"] == host["table"]
    assert plain["subject"] == tiny["subject"] == host["subject"] and plain["score"] == tiny["score"] == host["score"]


def mixed_set(seed=2):
    rng = np.random.default_rng(seed)
    lens = [int(x) for x in rng.integers(5, 101, 24)] + [int(x) for x in rng.integers(LIM["rows"][0] + 1, LIM["rows"][1] + 1, 9)] + \
           [int(x) for x in rng.integers(LIM["rows"][1] + 1, LIM["rows"][2] + 1, 5)] + [LIM["rows"][2] + 90, 1, 0]
    base = [random_protein(rng, n) for n in lens]
    genomes = []
    for g in range(3):
        order = rng.permutation(len(base))
        genomes.append([("g%d_p%d some title" % (g, i), mutate(rng, base[i], 0.08)) for i in order])
    return genomes


def test_mixed_set_and_counters(gpu_ctx):
    genomes = mixed_set()
    host = engine.sw_search_host(genomes)
    before = gpu_ctx.sw_stats()
    dev = gpu_ctx.sw_search(genomes)
    after = gpu_ctx.sw_stats()
    assert dev["table"] == host["table"] and len(host["query"]) > 100
    for k in ("query", "subject", "target_genome", "score", "bits", "evalue"):
        assert dev[k] == host[k], k
    total = sum(len(s) for g in genomes for _, s in g)
    assert dev["cells"] == host["cells"] == total * total
    assert after["cells"] - before["cells"] == total * total
    assert all(b > a for a, b in zip(before["launches"], after["launches"]))          # every class ran
    small = [g[:6] for g in genomes]
    assert gpu_ctx.sw_search(small, traceback=True, evalue=10.0)["table"] == engine.sw_search_host(small, traceback=True, evalue=10.0)["table"]
    with pytest.raises(engine.PmlError) as e:
        gpu_ctx.sw_search([[("a", "AC-A")]])
    assert e.value.code == engine.EINVAL and "position 2" in str(e.value)


def test_genome_files_to_set_files(gpu_ctx, tmp_path):
    genomes = planted_families()
    files = []
    for g, genome in enumerate(genomes):
        path = tmp_path / ("genome%d.faa" % g)
        path.write_text("".join(">%s\n%s\n%s\n\nA\n" % (title, res[:25], res[25:]) for title, res in genome))    # lines of length <= 1 are dropped
        files.append(str(path))
    search = tree_builder.HomologySearch(files, evalue=0.1, run_name="e1", ctx=gpu_ctx, out_dir=str(tmp_path))
    hits = search.getResults()
    assert hits == str(tmp_path / "e1_all_blast.out")
    assert open(hits, "rb").read() == engine.sw_search_host(genomes)["table"]
    hg = tree_builder.HomologGroups(hits, files, ctx=gpu_ctx, run_name="e1", out_dir=str(tmp_path))
    hg.run()
    sets = sorted(os.listdir(tmp_path / "hg_e1"))
    assert sets == ["set_0.faa", "set_1.faa", "set_2.faa"]
    families = []
    for name in sets:
        text = (tmp_path / "hg_e1" / name).read_text()
        families.append(sorted(ln[1:].split(" ")[0] for ln in text.split("\n") if ln.startswith(">")))
    assert sorted(families) == [sorted("g%d_f%d" % (g, f) for g in range(3)) for f in range(3)]
    import pepr_homolog_groups
    out = tmp_path / "tool"
    out.mkdir()
    assert pepr_homolog_groups.main(["-homology_search_method", "blast", "-genome_file"] + files + ["-run_name", "e2", "-out_dir", str(out)], ctx=gpu_ctx) == 0
    assert (out / "e2_all_blast.out").read_bytes() == open(hits, "rb").read()
    for name in sets:
        assert (out / "hg_e2" / name).read_text() == (tmp_path / "hg_e1" / name).read_text()
    import pepr_homology_search
    assert pepr_homology_search.main(["-genome_file"] + files + ["-o", str(out / "hits.m8")], ctx=gpu_ctx) == 0
    assert (out / "hits.m8").read_bytes() == open(hits, "rb").read()
