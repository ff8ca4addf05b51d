"""The homology search on the device (csrc/sw.hip) against the host twin and tests/sw_ref.py, exactly: every class through the test
door at its strip, group and pass boundaries, the stream's resets, ties across chunks and units, a mixed set, the counters
and the whole step from genome files to set files; then what BLOSUM62 and one chunk cannot see: tables that are not their own
transpose with entries at both ends of int8, gap costs of 2^20, several passes across chunks, chunk ranges and units, chunk lengths
around the 64-position batch, the cut at the default chunk size, the HBM-budget paths, a query of 65 535 rows, a pair without a
positive cell, and the selection keys against the raw scores.  Every expected score is sw_ref's."""
import os
import sys

import numpy as np
import pytest

from pepr_amd import engine, tree_builder
import sw_ref as ref
from sw_ref import NO_P, PLAIN, asym_tables, flanked, gap_subjects, mutate, planted_families, random_protein, stream_chunks

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIM = engine.sw_class_limits()
T = LIM["strip"]
ROWS = LIM["rows"][2]            # rows of one pass of the widest class
BATCH = 64                       # stream positions the kernel stages at a time (and reads of the line buffer)
ENOMEM = -4
BIG_COST = 1 << 20               # the largest gap cost the rule takes
_SEEN = {}                       # reference scores by sequence pair and options: copies of a sequence cost one evaluation


def ref_scores(queries, subjects, **opts):
    tag = tuple(sorted((k, v.tobytes() if isinstance(v, np.ndarray) else v) for k, v in opts.items()))
    out = np.zeros((len(queries), len(subjects)), dtype=np.int32)
    for i, q in enumerate(queries):
        for j, s in enumerate(subjects):
            key = (q.upper(), s.upper(), tag)
            if key not in _SEEN:
                _SEEN[key] = ref.score(q, s, **opts)
            out[i, j] = _SEEN[key]
    return out


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


# ---- what BLOSUM62 and one chunk cannot see ----
COSTS = ((BIG_COST, BIG_COST), (1, BIG_COST), (BIG_COST, 1), (1, 1))


def class2_growth(ctx, call):
    before = ctx.sw_stats()["launches"][2]
    out = call()
    return out, ctx.sw_stats()["launches"][2] - before


@pytest.mark.parametrize("cls", [0, 1, 2])
def test_asymmetric_and_extreme_tables(gpu_ctx, cls):
    """table[query][subject], entries of 127 and -128: a device table read the other way round passes every BLOSUM62 test"""
    rows = LIM["rows"][cls]
    rng = np.random.default_rng(60 + cls)
    lens = [T + 1, rows - 1] + ([rows + 7] if cls == 2 else [])                       # rows + 7: two passes
    queries = [random_protein(rng, n) for n in lens[:-1]] + [random_protein(rng, lens[-1], PLAIN)]
    long_q = queries[-1]
    telling = [random_protein(rng, 50), random_protein(rng, 120)]                     # two unrelated proteins ...
    telling += [mutate(rng, long_q[a:a + 60], 0.3) for a in (0, 30, len(long_q) - 60)]    # ... and short relatives: mismatches inside the alignment
    subjects = telling + [mutate(rng, q, 0.3) for q in queries]
    subjects += gap_subjects(long_q, T) + gap_subjects(long_q, 5 * T) + (gap_subjects(long_q, rows) if cls == 2 else [])
    for name, t in zip(("mild", "wild"), asym_tables()):
        want = ref_scores(queries, subjects, table=t)
        turned = ref_scores(queries[1:], telling, table=np.ascontiguousarray(t.T))    # (the short query and the exact pieces say little)
        share = float((turned != want[1:, :len(telling)]).mean())
        got = gpu_ctx.debug_sw_scores(queries, subjects, force_class=cls, table=t)
        print("class", cls, name, "table: the transpose changes %.2f of the telling subjects' scores; max |device - ref| =" % share, int(np.abs(got - want).max()))
        assert share >= 0.5                                                            # these inputs tell a table from its transpose
        assert (got == want).all(), (name, np.argwhere(got != want)[:8])


def test_asymmetric_table_through_search(gpu_ctx):
    rng = np.random.default_rng(66)
    mild = asym_tables()[0]
    base = [random_protein(rng, n) for n in (30, 45, 60, 140)]
    genomes = [[("a%d" % i, mutate(rng, s, 0.3)) for i, s in enumerate(base)], [("b%d x" % i, mutate(rng, s, 0.3)) for i, s in enumerate(base[::-1])]]
    e = ref.search(genomes, table=mild, evalue=10.0)
    assert e["margin"] > 1e-6 and len(e["hits"]) >= 12
    assert ref.search(genomes, table=np.ascontiguousarray(mild.T), evalue=10.0)["table"] != e["table"]
    host = engine.sw_search_host(genomes, table=mild, evalue=10.0)
    dev = gpu_ctx.sw_search(genomes, table=mild, evalue=10.0)
    assert dev["table"] == host["table"] == e["table"]
    assert list(zip(dev["query"], dev["subject"], dev["target_genome"], dev["score"])) == [h[:4] for h in e["hits"]]


@pytest.mark.parametrize("cls", [0, 1, 2])
def test_gap_costs_at_the_documented_limit(gpu_ctx, cls):
    """costs of 2^20 beside the 2^28 a boundary step subtracts"""
    rows = LIM["rows"][cls]
    rng = np.random.default_rng(70 + cls)
    queries = [random_protein(rng, rows - 1, PLAIN)] + ([random_protein(rng, rows + 40, PLAIN)] if cls == 2 else [])
    long_q = queries[-1]
    subjects = gap_subjects(long_q, 5 * T, flank=30) + (gap_subjects(long_q, rows, flank=30) if cls == 2 else [])     # the pass boundary faces a gap
    subjects += [mutate(rng, queries[0][:100], 0.1), random_protein(rng, BATCH + 1)]
    want = {}
    for go, ge in COSTS:
        want[go, ge] = ref_scores(queries, subjects, gap_open=go, gap_extend=ge)
        got = gpu_ctx.debug_sw_scores(queries, subjects, force_class=cls, gap_open=go, gap_extend=ge)
        print("class", cls, "costs", (go, ge), "max |device - ref| =", int(np.abs(got - want[go, ge]).max()))
        assert (got == want[go, ge]).all(), ((go, ge), np.argwhere(got != want[go, ge])[:8])
    ngap = 4 if cls == 2 else 2
    assert (want[1, 1][-1, :ngap] > want[BIG_COST, BIG_COST][-1, :ngap]).all()         # the planted gaps are taken when they are cheap
    for opts in ({"gap_open": BIG_COST + 1}, {"gap_extend": BIG_COST + 1}):
        with pytest.raises(engine.PmlError) as e:
            gpu_ctx.debug_sw_scores(queries[:1], subjects[:1], force_class=cls, **opts)
        assert e.value.code == engine.EINVAL


def test_several_passes_across_chunks_ranges_and_units(gpu_ctx, monkeypatch):
    """line buffers at a chunk's offset inside its range, rewritten range after range, for units that split a list of queries of
    several passes"""
    rng = np.random.default_rng(77)
    p = random_protein(rng, 3 * ROWS + 5, PLAIN)
    queries = [mutate(rng, p[:ROWS + 1], 0.1), mutate(rng, p[:2 * ROWS], 0.1), mutate(rng, p[:2 * ROWS + 1], 0.1), p]
    queries += [queries[1], p[ROWS - 50:ROWS + 50], p[2 * ROWS - 150:2 * ROWS + 150]]  # a copy of the second; two of one pass
    npass = [(len(q) + ROWS - 1) // ROWS for q in queries]
    assert npass == [2, 2, 3, 4, 2, 1, 1] and LIM["rows"][1] < len(queries[-1]) <= ROWS
    # the widest class's list by length is 300, R + 1, 2R, 2R | 2R + 1, 3R + 5: the second unit of three holds line-buffer slots 0, 1, 2
    lens = [1, 2, 38, 39, 40, 41, 63, 64, 65, 90, 127, 128, 129, 200]
    subjects = []
    for k, n in enumerate(lens):
        at = min(ROWS * (1 + k % 3) - n // 2, len(p) - n)                              # across a pass boundary of the longest query
        subjects.append(mutate(rng, p[at:at + n], 0.1))
    subjects += gap_subjects(p, ROWS) + gap_subjects(p, 2 * ROWS)                      # the pass boundaries carry a gap
    subjects = [subjects[i] for i in rng.permutation(len(subjects))]
    assert sorted(len(s) for s in subjects)[-14 + 2:] == lens[2:] and [len(s) for s in subjects] != sorted(len(s) for s in subjects)
    sizes, _ = stream_chunks([len(s) for s in subjects], 40)
    assert len(sizes) >= 12                                                            # at least six ranges of two chunks
    want = ref_scores(queries, subjects)
    genomes = [[("s%d" % i, s) for i, s in enumerate(subjects)], [("q%d" % i, q) for i, q in enumerate(queries)]]
    host = engine.sw_search_host(genomes)
    monkeypatch.setenv("PML_SW_TINY_UNITS", "1")
    got, grown = class2_growth(gpu_ctx, lambda: gpu_ctx.debug_sw_scores(queries, subjects))
    print("max |device - ref| =", int(np.abs(got - want).max()), "launches of the widest class:", grown)
    assert (got == want).all(), np.argwhere(got != want)[:8]
    assert grown >= 6                                                                  # at least two units times at least three ranges
    dev = gpu_ctx.sw_search(genomes)
    assert dev["table"] == host["table"] and len(host["query"]) >= len(queries)
    for k in ("query", "subject", "target_genome", "score"):
        assert dev[k] == host[k], k
    assert (gpu_ctx.debug_sw_scores(queries, subjects) == want).all()                 # the same context again: the buffer is reused
    assert gpu_ctx.sw_search(genomes)["table"] == host["table"]


def test_stream_lengths_around_the_batch(gpu_ctx, monkeypatch):
    """chunks of 60 .. 71 and 124 .. 133 stream bytes: one short of, at and one past the 64 positions staged at a time"""
    rng = np.random.default_rng(81)
    p = random_protein(rng, ROWS + 1, PLAIN)
    lens = list(range(59, 71)) + list(range(123, 133))
    subjects = [mutate(rng, p[len(p) - n:-1], 0.1) + p[-1] for n in lens]              # they end on the second pass's only row
    subjects = [subjects[i] for i in rng.permutation(len(subjects))]
    sizes, _ = stream_chunks([len(s) for s in subjects], 40)
    assert sizes == [n + 1 for n in lens]                                              # every subject is a chunk alone
    assert {BATCH - 1, BATCH, BATCH + 1, 2 * BATCH - 1, 2 * BATCH, 2 * BATCH + 1} <= set(sizes)
    short = p[-(T + 1):]
    monkeypatch.setenv("PML_SW_TINY_UNITS", "1")
    for cls in range(3):
        got = gpu_ctx.debug_sw_scores([short], subjects, force_class=cls)
        assert (got == ref_scores([short], subjects)).all(), cls
    want = ref_scores([p], subjects)
    got = gpu_ctx.debug_sw_scores([p], subjects, force_class=2)                        # two passes: batched reads of the line buffer
    print("max |device - ref| =", int(np.abs(got - want).max()))
    assert (got == want).all(), np.argwhere(got != want)[:8]


_CASE = {}


def copies_case():
    """40 subjects near 300 residues out of three sequences (free of P), the longer ones first in the file so that stream order
    is not file order; four queries, one of each class and one of two passes, that tie on the copies of a sequence"""
    if not _CASE:
        rng = np.random.default_rng(91)
        bases = [random_protein(rng, 304, NO_P) for _ in range(3)]
        subjects = [bases[k % 3][:304 if k < 12 else 296] for k in range(40)]
        a, b, c = bases
        queries = [a[:100], b[50:250], c[5:291], a[:290] + random_protein(rng, 310, NO_P)]
        assert [len(q) <= r for q, r in zip(queries, LIM["rows"])] == [True] * 3 and LIM["rows"][1] < len(queries[2]) and ROWS < len(queries[3]) <= 2 * ROWS
        _CASE.update(rng=rng, bases=bases, subjects=subjects, queries=queries)
    return _CASE


def test_default_chunk_cutting(gpu_ctx):
    """no hook: the cut at the default chunk size, copies of a sequence on both sides of it, a subject longer than a chunk"""
    case = copies_case()
    queries, subjects = case["queries"], list(case["subjects"])
    core = mutate(np.random.default_rng(92), queries[3][240:340], 0.1)                 # across the two-pass query's pass boundary
    long_s = flanked(core, LIM["chunk"] + 100, 5000)
    subjects.insert(20, long_s)
    alone = list(subjects)
    alone[20] = core                                                                   # the flank identity: the queries hold no P
    assert not any("P" in q for q in queries)
    sizes, where = stream_chunks([len(s) for s in subjects], LIM["chunk"])
    assert sum(sizes) > 2 * LIM["chunk"] and len(sizes) >= 3 and sizes[where[20]] == len(long_s) + 1 > LIM["chunk"]
    twins = [k for k, s in enumerate(subjects) if s == subjects[-1]]
    assert len({where[k] for k in twins}) > 1                                          # identical copies in different chunks
    assert where[0] > where[21] and len(subjects[0]) > len(subjects[21])               # the first in the file comes late in the stream
    want = ref_scores(queries, alone)
    got = gpu_ctx.debug_sw_scores(queries, subjects)
    print("max |device - ref| =", int(np.abs(got - want).max()))
    assert (got == want).all(), np.argwhere(got != want)[:8]
    genomes = [[("s%d" % i, s) for i, s in enumerate(subjects)], [("q%d" % i, q) for i, q in enumerate(queries)]]
    host = engine.sw_search_host(genomes)
    dev = gpu_ctx.sw_search(genomes)
    assert dev["table"] == host["table"]
    for k in ("query", "subject", "target_genome", "score"):
        assert dev[k] == host[k], k
    won = {q - len(subjects): (s, sc) for q, s, g, sc in zip(dev["query"], dev["subject"], dev["target_genome"], dev["score"]) if g == 0 and q >= len(subjects)}
    for i in range(len(queries)):
        ties = np.flatnonzero(want[i] == want[i].max())
        assert len(ties) >= 13 and len({where[int(k)] for k in ties}) > 1                # the copies tie, across chunks
        assert won[i] == (int(ties[0]), int(want[i].max())) and ties[0] == (0, 1, 2, 0)[i]     # the lowest file position wins


def resident_bytes(qlens, slens, dbg=True, G=1):
    """what score_all (csrc/sw.cpp) keeps on the device beside the line buffers, array by array, each rounded up to 256 bytes; the
    query and chunk records of kernels.h are 24 bytes each"""
    up = lambda n: (n + 255) // 256 * 256       # noqa: E731
    nq, ns = len(qlens), len(slens)
    sizes, _ = stream_chunks(slens, LIM["chunk"])
    return (up(nq * G * 8) + up(nq * 24) + up(len(sizes) * 24) + up(ns * 4) + (up(nq * ns * 4) if dbg else 0) + up(25 * 32) + up(max(sum(qlens), 1)) +
            up(sum(sizes)))


def test_hbm_budget_paths(gpu_ctx, monkeypatch):
    """the unit split by the line buffers' share of the budget, and the refusal of a stream whose one line buffer does not fit"""
    case = copies_case()
    subjects = case["subjects"]
    two = case["queries"][3]
    three = case["bases"][1][:296] + random_protein(np.random.default_rng(93), 2 * ROWS + 6 - 296, NO_P)
    queries = [two, three, two, two, three, two, three]
    assert sorted({(len(q) + ROWS - 1) // ROWS for q in queries}) == [2, 3]
    slens = [len(s) for s in subjects]
    stream = sum(slens) + len(slens)
    assert 11000 < stream < 13000 and stream < (1 << 20)                              # one chunk range: a line buffer is `stream` int2
    budget = 1 << 20
    off = resident_bytes([len(q) for q in queries], slens)
    slots = min((budget - off) // 2, 1 << 30) // (stream * 8)                          # line buffers a unit may hold
    units = -(-len(queries) // slots)
    assert 1 <= slots < len(queries) and units >= 2
    want = ref_scores(queries, subjects)
    got, plain = class2_growth(gpu_ctx, lambda: gpu_ctx.debug_sw_scores(queries, subjects))
    assert (got == want).all() and plain == 1
    monkeypatch.setenv("PML_HBM_BUDGET_MB", "1")
    got, grown = class2_growth(gpu_ctx, lambda: gpu_ctx.debug_sw_scores(queries, subjects))
    print("line-buffer slots per unit", slots, "launches", grown, "against", plain, "max |device - ref| =", int(np.abs(got - want).max()))
    assert (got == want).all(), np.argwhere(got != want)[:8]
    assert grown == units > plain
    many = [subjects[k % len(subjects)] for k in range(250)]
    mlens = [len(s) for s in many]
    mstream = sum(mlens) + len(mlens)
    need = resident_bytes([len(two)], mlens) + 2 * mstream * 8
    assert mstream > 70000 and need > budget * 1.15
    before = gpu_ctx.sw_stats()
    with pytest.raises(engine.PmlError) as e:
        gpu_ctx.debug_sw_scores([two], many)
    assert e.value.code == ENOMEM and "MiB of HBM" in str(e.value) and "%d subject residues" % mstream in str(e.value)
    assert gpu_ctx.sw_stats() == before                                               # no kernel ran
    monkeypatch.delenv("PML_HBM_BUDGET_MB")
    assert (gpu_ctx.debug_sw_scores([two], many[:3]) == ref_scores([two], many[:3])).all()


def test_the_longest_query(gpu_ctx):
    """65 535 rows: 128 passes of the widest class"""
    limit = 65535
    assert (limit + ROWS - 1) // ROWS == 128
    rng = np.random.default_rng(97)
    core = random_protein(rng, 100, NO_P)
    at = 100 * ROWS - 50                                                               # the core across a pass boundary far in
    q = flanked(core, limit, at)
    subjects = gap_subjects(core, 50, flank=30) + [mutate(rng, core, 0.2).replace("P", "A"), random_protein(rng, 70, NO_P), random_protein(rng, 131, NO_P)]
    assert not any("P" in s for s in subjects)
    want = ref_scores([core], subjects)
    got = gpu_ctx.debug_sw_scores([q], subjects)
    print("device", got[0].tolist(), "ref", want[0].tolist())
    assert (got == want).all() and want[0, :3].min() > 100
    w = "W" * limit
    assert gpu_ctx.debug_sw_scores([w], ["W" * 300, "W"])[0].tolist() == [3300, 11]
    assert ref.score("W" * 300, "W" * 300) == 3300 and ref.score("W" * 40, "W") == 11
    with pytest.raises(engine.PmlError) as e:
        gpu_ctx.debug_sw_scores([w + "W"], ["W"])
    assert e.value.code == engine.EINVAL and "65535" in str(e.value)


def test_no_positive_cell(gpu_ctx):
    """W against P scores -4: a (query, genome) without a positive cell has no line"""
    ws, ps = ["W" * n for n in (T + 1, LIM["rows"][0] + 30, LIM["rows"][1] + 30, ROWS + 30)], ["P" * n for n in (1, 5, 50, BATCH + 1)]
    genomes = [[("p%d" % i, s) for i, s in enumerate(ps)], [("w%d" % i, s) for i, s in enumerate(ws)]]
    e = ref.search(genomes)
    host = engine.sw_search_host(genomes)
    dev = gpu_ctx.sw_search(genomes)
    assert e["margin"] > 1e-6 and dev["table"] == host["table"] == e["table"]
    pairs = set(zip(dev["query"], dev["target_genome"]))
    assert pairs == set(zip(host["query"], host["target_genome"]))
    assert not any((len(ps) + i, 0) in pairs for i in range(len(ws))) and not any((i, 1) in pairs for i in range(len(ps)))
    assert all((len(ps) + i, 1) in pairs for i in range(len(ws)))                      # the W's own genome: the self hits
    for cls in (-1, 2):
        assert not gpu_ctx.debug_sw_scores(ws, ps, force_class=cls).any()
    assert not ref_scores(ws[:1], ps).any()


@pytest.mark.parametrize("tiny", [0, 1])
def test_keys_against_the_door(gpu_ctx, monkeypatch, tiny):
    """the selection key of every query is the first arg-max of the query's row of raw scores"""
    rng = np.random.default_rng(101)
    p = random_protein(rng, 15, PLAIN)
    r = random_protein(rng, 40, PLAIN)
    fill = lambda n: random_protein(rng, n, "GS")       # noqa: E731
    target = [fill(9), r, p + "PPP", fill(30), fill(12), p, fill(20), r, fill(5), p, fill(33), "GG" + p, r + "GS", fill(3), p, fill(17), r]
    queries = [p, fill(10), p.lower(), r[:30], r + fill(200), fill(300), p + fill(ROWS + 10)]
    allp = target + queries
    want = ref_scores(allp, target)
    if tiny:
        monkeypatch.setenv("PML_SW_TINY_UNITS", "1")
    raw = gpu_ctx.debug_sw_scores(allp, target)
    assert (raw == want).all()
    dev = gpu_ctx.sw_search([[("t%d" % i, s) for i, s in enumerate(target)], [("q%d" % i, s) for i, s in enumerate(queries)]], evalue=1e300)
    won = {q: (s, sc) for q, s, g, sc in zip(dev["query"], dev["subject"], dev["target_genome"], dev["score"]) if g == 0}
    assert sorted(won) == [q for q in range(len(allp)) if raw[q].max() > 0] and len(won) == len(allp)
    for q, (s, sc) in won.items():
        assert (s, sc) == (int(np.argmax(raw[q])), int(raw[q].max())), q
    tied = [q for q in won if (raw[q] == raw[q].max()).sum() > 1]
    assert len(tied) >= 6 and any(won[q][0] != q for q in tied if q < len(target))     # planted ties, and a copy that loses to an earlier one
