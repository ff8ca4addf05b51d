"""The MinHash path on the device (k_mash_hash, the selection, k_mash_pairs, pml_neighbor_masher) against the restatement of the
published rule and of the Java's selection (mash_ref.py).  Every integer is compared for equality; so are the distances at six
digits; raw doubles within 2 ulp (two rounded operations and a log of an unpinned libm)."""
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from pepr_amd import engine, tree_builder
import mash_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "mash_cases.json")))
T = engine.mash_tile()               # window starts k_mash_hash stages at a time
W = engine.mash_chunk()              # sketch values k_mash_pairs takes at a time
KS = (1, 8, 9, 15, 16, 17, 21, 31, 32)
BASES = np.frombuffer(b"ACGT", dtype=np.uint8)


def bases(rng, n):
    return BASES[rng.integers(0, 4, n)].tobytes()


def mutate(rng, g, rate):
    a = np.frombuffer(g, dtype=np.uint8).copy()
    hit = rng.random(a.size) < rate
    shift = rng.integers(1, 4, a.size)
    idx = np.searchsorted(BASES, a)                # ACGT is ascending
    a[hit] = BASES[(idx[hit] + shift[hit]) % 4]
    return a.tobytes()


def same_sketches(got, genomes, k, s):
    assert len(got) == len(genomes)
    for g, (have, genome) in enumerate(zip(got, genomes)):
        want = ref.sketch(genome, k, s)
        assert have.dtype == np.uint64 and have.shape == want.shape and (have == want).all(), (g, k, s, have[:5], want[:5])


def within_2ulp(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool((np.abs(a - b) <= 2 * np.spacing(np.maximum(np.abs(a), np.abs(b)))).all())


# ---- k_mash_hash ----
@pytest.mark.parametrize("k", KS)
def test_hash_record_lengths_around_k_and_the_tile(gpu_ctx, k):
    rng = np.random.default_rng(100 + k)
    genome = [bases(rng, n) for n in (k - 1, k, k + 1, T - 1, T, T + 1, 2 * T + k - 2)]
    got = gpu_ctx.debug_mash_hashes(genome, k)
    assert (got == ref.hashes(genome, k)).all()
    assert (got == engine.mash_hashes_host(genome, k)).all()
    if k in (1, 17):                               # the plain-int restatement on the short records
        short = genome[:3]
        slow = [v for r in short for v in ref.record_values_slow(r, k)]
        assert [int(x) for x in got[:len(slow)]] == slow


@pytest.mark.parametrize("k", (1, 9, 16, 21, 32))
def test_hash_invalid_bytes_lower_case_and_boundaries(gpu_ctx, k):
    rng = np.random.default_rng(200 + k)
    first = bytearray(bases(rng, T - 1))           # with its separator exactly one tile: the second record starts on a tile boundary
    body = bytearray(bases(rng, 3 * T + 5))
    for pos, byte in ((0, b"N"), (k - 1, b"n"), (T - 1, b"-"), (T, b"\x00"), (2 * T - k, b"\xff"), (2 * T + 1, b"R"), (T + 200, b"@"), (T + 300, b"["),
                      (T + 400, b"`"), (T + 500, b"{"), (T + 600, b"U"), (T + 700, b"\n")):
        body[pos:pos + 1] = byte
    lower = bases(rng, 300).lower()
    mixed = bytes(b | 0x20 if i % 3 == 0 else b for i, b in enumerate(bases(rng, 300)))
    pal = b"ACGT" * 20 + b"AATT" * 10 + b"GAATTC" * 8          # windows equal to their own reverse complement (even k)
    genome = [bytes(first), bytes(body), b"", bases(rng, max(k - 1, 0)), lower, mixed, pal, b"N" * 40, bases(rng, 5)]
    got = gpu_ctx.debug_mash_hashes(genome, k)
    want = ref.hashes(genome, k)
    assert (got == want).all(), np.nonzero(got != want)[0][:10]
    if k == 1:
        assert int((got != ref.INVALID).sum()) > 3 * T       # and the marks are where the non-ACGT bytes are
    up = [r.upper() for r in genome]
    assert (gpu_ctx.debug_mash_hashes(up, k)[:T - 1] == got[:T - 1]).all()
    lo, hi = T - 1 + 3 * T + 5 + max(k - 1, 0), T - 1 + 3 * T + 5 + max(k - 1, 0) + 300
    assert (gpu_ctx.debug_mash_hashes([lower.upper()], k) == got[lo:hi]).all()          # lower case reads as upper case


def test_hash_canonical_4mers(gpu_ctx):
    import itertools
    recs = ["".join(p) for p in itertools.product("ACGT", repeat=4)]
    got = gpu_ctx.debug_mash_hashes(recs, 4)
    vals = got[got != ref.INVALID]
    assert vals.size == 256 and np.unique(vals).size == GOLD["canonical_4mers"]["distinct"] == 136
    assert int(vals.max()) < 1 << 32                                                     # k <= 16 keeps 32 bits
    one = "".join(recs)                                                                  # one record holding every 4-mer start
    assert len(gpu_ctx.mash_sketch([[one + one[:3]]], 4, 1000)[0]) <= 136


# ---- sketches ----
def test_sketch_few_distinct_values(gpu_ctx):
    rng = np.random.default_rng(3)
    motif = bases(rng, 50)
    genomes = [[motif * 40], [bases(rng, 700)] * 2, [motif * 3, motif * 3]]
    for s in (1, 10, 100, 1000):
        same_sketches(gpu_ctx.mash_sketch(genomes, 21, s), genomes, 21, s)


def test_sketch_sizes_around_the_distinct_count(gpu_ctx):
    rng = np.random.default_rng(4)
    genome = [bases(rng, 320)]
    D = np.unique(ref.genome_values(genome, 21)).size
    assert 250 < D <= 300
    for s in (D + 5, D + 1, D, D - 1, 1):
        got = gpu_ctx.mash_sketch([genome], 21, s)
        same_sketches(got, [genome], 21, s)
        assert len(got[0]) == min(s, D)


def test_sketch_heavy_duplicates_and_32_bit_values(gpu_ctx):
    rng = np.random.default_rng(5)
    g4 = [bases(rng, 6000)]
    got = gpu_ctx.mash_sketch([g4], 4, 100)
    same_sketches(got, [g4], 4, 100)
    assert len(got[0]) == 100
    assert len(gpu_ctx.mash_sketch([g4], 4, 137)[0]) == 136                              # everything there is
    g11 = [bases(rng, 40000)]
    for s in (500, 30000):
        same_sketches(gpu_ctx.mash_sketch([g11], 11, s), [g11], 11, s)
    same_sketches(gpu_ctx.mash_sketch([g11], 16, 2000), [g11], 16, 2000)


def test_sketch_cut_search_and_take_everything(gpu_ctx):
    rng = np.random.default_rng(6)
    g = [bases(rng, 200000)]
    before = gpu_ctx.mash_stats()
    same_sketches(gpu_ctx.mash_sketch([g], 21, 1000), [g], 21, 1000)
    mid = gpu_ctx.mash_stats()
    assert mid["repeats"] == before["repeats"] and mid["hash_launches"] == before["hash_launches"] + 1      # the first cut was enough
    same_sketches(gpu_ctx.mash_sketch([g], 21, 150000), [g], 21, 150000)
    got = gpu_ctx.mash_sketch([g], 21, 199000)                                           # more than the histogram can promise: everything is taken
    same_sketches(got, [g], 21, 199000)
    assert len(got[0]) == 199000
    gpu_ctx.debug_mash_full_sort(True)                                                   # the baseline gives the same sketch
    try:
        same_sketches(gpu_ctx.mash_sketch([g], 21, 1000), [g], 21, 1000)
    finally:
        gpu_ctx.debug_mash_full_sort(False)


def test_sketch_batch_of_different_lengths_and_split_by_budget(gpu_ctx, monkeypatch):
    rng = np.random.default_rng(7)
    genomes = [[bases(rng, 100)], [bases(rng, 5000), b"", bases(rng, 30)], [bases(rng, 70000)], [], [bases(rng, 20)], [b"NNNN" * 10],
               [bases(rng, 15000)], [bases(rng, 15000)], [bases(rng, 15000)]]
    whole = gpu_ctx.mash_sketch(genomes, 21, 300)
    same_sketches(whole, genomes, 21, 300)
    assert [len(x) for x in whole][3:6] == [0, 0, 0]
    before = gpu_ctx.mash_stats()["hash_launches"]
    monkeypatch.setenv("PML_HBM_BUDGET_MB", "2")                                         # 70 000 bases need 1.7 MiB: a sub-batch of their own
    split = gpu_ctx.mash_sketch(genomes, 21, 300)
    assert gpu_ctx.mash_stats()["hash_launches"] >= before + 2
    assert all((a == b).all() for a, b in zip(whole, split))
    d = gpu_ctx.mash_distances(genomes[:3], genomes[6:], 21, 300)
    monkeypatch.setenv("PML_HBM_BUDGET_MB", "1")
    with pytest.raises(engine.PmlError) as e:
        gpu_ctx.mash_sketch(genomes, 21, 300)
    assert e.value.code == -4 and "genome 2" in str(e.value)
    monkeypatch.delenv("PML_HBM_BUDGET_MB")
    d2 = gpu_ctx.mash_distances(genomes[:3], genomes[6:], 21, 300)
    assert all((d[key] == d2[key]).all() for key in d)


# ---- k_mash_pairs ----
def check_pairs(ctx, A, B, k, s):
    r = ctx.mash_dist(A, B, k, s, digits=None)
    r6 = ctx.mash_dist(A, B, k, s, digits=6)
    for i, a in enumerate(A):
        for j, b in enumerate(B):
            c, d = ref.pair(a, b, s)
            assert (int(r["common"][i, j]), int(r["denom"][i, j])) == (c, d), (i, j, s, len(a), len(b))
            assert ref.pair_fast(a, b, s) == (c, d)
            assert within_2ulp(r["distance"][i, j], ref.distance(c, d, k))
            assert r6["distance"][i, j] == ref.distance(c, d, k, 6)
            if c == d or c == 0:
                assert r["distance"][i, j] == (0.0 if c == d else 1.0)
    return r


def test_pairs_lengths_around_the_chunk(gpu_ctx):
    rng = np.random.default_rng(8)
    universe = np.unique(rng.integers(0, 1 << 63, 3 * W + 50, dtype=np.uint64))
    lens = (W - 1, W, W + 1, 2 * W + 3, 0, 1, 5)
    A = [np.sort(rng.choice(universe, n, replace=False)) for n in lens]
    B = [np.sort(rng.choice(universe, n, replace=False)) for n in lens]
    for s in (2 * W + 3, W + 1, W, 5):
        check_pairs(gpu_ctx, [a[:s] for a in A], [b[:s] for b in B], 21, s)


def test_pairs_the_sth_union_element_on_a_chunk_boundary(gpu_ctx):
    n = 2 * W + 8
    for at in (W - 1, W, 2 * W - 1, 2 * W):                     # the shared value is a's element `at`: last of a chunk, first of the next
        a = np.arange(n, dtype=np.uint64) * 2 + 10              # even values
        b = np.arange(n, dtype=np.uint64) * 2 + 11              # odd values, one between every two of a
        b = np.sort(np.append(b[b != a[at] + 1], a[at]))        # a[at] is shared; its union rank is 2 at
        rank = 2 * at
        assert ref.pair(a, b, rank + 1)[0] == 1 and ref.pair(a, b, rank)[0] == 0
        for s in (rank + 1, rank, rank + 2, rank - 1):          # counted as the s-th, not as the (s+1)-th
            r = check_pairs(gpu_ctx, [a[:s]], [b[:s]], 21, s)
            if len(a[:s]) > at and a[at] in b[:s]:
                assert int(r["common"][0, 0]) == (1 if s >= rank + 1 else 0)


def test_pairs_identical_disjoint_empty_and_golden(gpu_ctx):
    rng = np.random.default_rng(9)
    x = np.unique(rng.integers(0, 1 << 64, 700, dtype=np.uint64))
    y = np.setdiff1d(np.unique(rng.integers(0, 1 << 64, 700, dtype=np.uint64)), x)
    e = np.zeros(0, dtype=np.uint64)
    s = 600
    r = check_pairs(gpu_ctx, [x[:s], y[:s], e], [x[:s], y[:s], e], 21, s)
    assert (int(r["common"][0, 0]), int(r["denom"][0, 0]), r["distance"][0, 0]) == (s, s, 0.0)
    assert (int(r["common"][0, 1]), int(r["denom"][0, 1]), r["distance"][0, 1]) == (0, s, 1.0)
    assert (int(r["common"][2, 2]), int(r["denom"][2, 2]), r["distance"][2, 2]) == (0, 0, 0.0)
    assert (int(r["common"][0, 2]), int(r["denom"][0, 2]), r["distance"][0, 2]) == (0, s, 1.0)
    for case in GOLD["pairs"]:
        a, b = np.array(case["a"], dtype=np.uint64), np.array(case["b"], dtype=np.uint64)
        r = gpu_ctx.mash_dist([a], [b], 21, case["s"], digits=None)
        assert (int(r["common"][0, 0]), int(r["denom"][0, 0])) == (case["common"], case["denom"]), case["name"]
        if "distance" in case:
            assert r["distance"][0, 0] == case["distance"], case["name"]
    with pytest.raises(engine.PmlError):
        gpu_ctx.mash_dist([np.array([3, 3], dtype=np.uint64)], [x[:5]], 21, 5)           # not distinct


def family(rng, n=3000):
    base = bases(rng, n)
    return base, [mutate(rng, base, r) for r in (0.0, 0.01, 0.05, 0.30)] + [bases(rng, n)]


def test_pairs_block_of_mutated_copies_takes_every_branch_of_the_distance(gpu_ctx):
    rng = np.random.default_rng(10)
    base, A = family(rng)
    B = [base] + [mutate(rng, base, r) for r in (0.0, 0.01, 0.02, 0.05, 0.30)] + [bases(rng, 3000)]
    A, B = [[g] for g in A], [[g] for g in B]
    k, s = 21, 200
    r = gpu_ctx.mash_distances(A, B, k, s, digits=None)
    ska, skb = [ref.sketch(g, k, s) for g in A], [ref.sketch(g, k, s) for g in B]
    for i in range(5):
        for j in range(7):
            c, d = ref.pair(ska[i], skb[j], s)
            assert (int(r["common"][i, j]), int(r["denom"][i, j])) == (c, d) and d == s
            assert within_2ulp(r["distance"][i, j], ref.distance(c, d, k))
    col = [int(x) for x in r["common"][:, 0]]                    # against the base: identical, ever fewer shared, none
    assert col[0] == s and s > col[1] > col[2] > col[3] >= 0 and col[4] == 0, col
    assert r["distance"][0, 0] == 0.0 and r["distance"][4, 0] == 1.0 and 0.0 < r["distance"][1, 0] < r["distance"][2, 0] < 1.0
    # the same from host sketches
    got = gpu_ctx.mash_sketch(A + B, k, s)
    r2 = gpu_ctx.mash_dist(got[:5], got[5:], k, s, digits=None)
    assert all((r[key] == r2[key]).all() for key in r)


# ---- pml_neighbor_masher ----
def masher_family():
    rng = np.random.default_rng(11)
    base = bases(rng, 3000)
    ingroup = [("in%d_@_I%d" % (i, i), [mutate(rng, base, r)]) for i, r in enumerate((0.005, 0.01, 0.015, 0.02))]
    pool = [("p%d_@_P%d" % (i, i), [mutate(rng, base, r)]) for i, r in enumerate((0.02, 0.03, 0.06, 0.08, 0.08, 0.10, 0.45))]
    pool.append(("far_@_P7", [bases(rng, 3000)]))
    return ingroup, pool


@pytest.mark.parametrize("opts", [dict(), dict(expand_ingroup=6), dict(expand_ingroup=6, digits=None), dict(expand_ingroup=4, outgroup_count=2),
                                  dict(expand_ingroup=6, ingroup_only=True), dict(expand_ingroup=6, outgroup_only=True), dict(expand_ingroup=20, outgroup_count=5),
                                  dict(expand_ingroup=1, outgroup_count=3)])
def test_neighbor_masher_equals_the_restated_run(gpu_ctx, opts):
    ingroup, pool = masher_family()
    k, s = 16, 400
    r = gpu_ctx.neighbor_masher(ingroup, pool, k=k, s=s, **opts)
    o = dict(opts)
    want = ref.run(ingroup, pool, k, s, outgroup_count=o.pop("outgroup_count", 3), expand=o.pop("expand_ingroup", 0), digits=o.pop("digits", 6), **o)
    assert r["ingroup"] == want["ingroup"] and r["outgroup"] == want["outgroup"] and r["taxa"] == want["taxa"]
    if opts.get("digits", 6):
        assert (r["distance"] == want["distance"]).all()
    else:
        assert within_2ulp(r["distance"], want["distance"])
    if not opts.get("ingroup_only"):
        for key in ("mean", "sd", "max"):
            assert within_2ulp(r[key], want[key]) or (r[key] != r[key] and want[key] != want[key]), key
        assert within_2ulp(r["candidate_distance"], want["candidate_distance"])
    n_out = len(r["outgroup"])
    assert (r["ingroup_tree"] is not None) == want["ingroup_tree_built"] and (r["rooted_tree"] is not None) == want["rooted_tree_built"]
    if r["ingroup_tree"] is not None:
        assert r["ingroup_tree"] == engine.nj_from_matrix(r["ingroup"], r["distance"][n_out:, n_out:], engine.NJ_DISTANCE, engine.NJ_TREE)
    if r["rooted_tree"] is not None:
        assert r["rooted_tree"] == engine.nj_from_matrix(r["taxa"], r["distance"], engine.NJ_DISTANCE, engine.NJ_TREE)
        assert r["taxa"][:n_out] == r["outgroup"]
    if opts.get("expand_ingroup") == 6 and not opts.get("ingroup_only"):
        assert len(r["ingroup"]) == 6 and 1 <= n_out <= 3 and r["ingroup_tree"] is not None or opts.get("outgroup_only")


def test_neighbor_masher_refusals(gpu_ctx):
    ingroup, pool = masher_family()
    for bad in (dict(k=0), dict(k=33), dict(s=0)):
        with pytest.raises(engine.PmlError) as e:
            gpu_ctx.neighbor_masher(ingroup, pool, **dict(dict(k=16, s=100), **bad))
        assert e.value.code == engine.EINVAL
    for ing, po, word in ((ingroup + [ingroup[0]], pool, "twice"), (ingroup, pool + [pool[1]], "twice"), ([], pool, "empty"), (ingroup, [], "empty"),
                          (ingroup, pool + [("short_@_S", [b"ACGT"])], "empty"), (ingroup + [("n_@_N", [b"N" * 100])], pool, "empty")):
        with pytest.raises(engine.PmlError) as e:
            gpu_ctx.neighbor_masher(ing, po, k=16, s=100)
        assert e.value.code == engine.EINVAL and word in str(e.value), str(e.value)
    with pytest.raises(engine.PmlError):
        gpu_ctx.mash_sketch([[b"ACGT"]], 33, 10)
    assert gpu_ctx.mash_sketch([[b"ACGT"]], 21, 10)[0].size == 0                          # the lower calls return an empty sketch
    r = gpu_ctx.neighbor_masher(ingroup, [], k=16, s=100, ingroup_only=True)             # no pool needed
    assert r["outgroup"] == [] and r["ingroup"] == [t[0] for t in ingroup]


def test_tool_writes_the_four_files(gpu_ctx, tmp_path):
    ingroup, pool = masher_family()

    def fasta(name, taxon, genome, extra=b""):
        path = str(tmp_path / name)
        with open(path, "wb") as f:
            f.write(b">acc1 chromosome [" + taxon.replace("_@_", " | ").encode() + b"]\n")          # ' | ' reads back as "_@_" (:104-111)
            seq = genome[0]
            for i in range(0, len(seq), 70):
                f.write(seq[i:i + 70] + b"\n")
            f.write(extra)
        return path
    # a second record in one file: the genome has two records
    extra = b">plasmid\nACGTTGCAACGTTGCAAGGTC\n"
    in_files = [fasta("in%d.fna" % i, t, g, extra if i == 0 else b"") for i, (t, g) in enumerate(ingroup)]
    pool_files = [fasta("p%d.fna" % i, t, g) for i, (t, g) in enumerate(pool)]
    ingroup = [(t, g if i else [g[0], b"ACGTTGCAACGTTGCAAGGTC"]) for i, (t, g) in enumerate(ingroup)]
    want = gpu_ctx.neighbor_masher(ingroup, pool, k=16, s=400, expand_ingroup=6, outgroup_count=2)
    run = str(tmp_path / "fam")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "pepr_neighbor_masher.py"), "-ingroup"] + in_files + ["-outgroup"] + pool_files +
                       ["-k", "16", "-s", "400", "-expand_ingroup", "6", "-outgroup_count", "2", "-run_name", run, "-mash", "/usr/bin/mash", "-p", "4"],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "-mash is ignored" in p.stderr and "-p is ignored" in p.stderr
    assert open(run + "_ingroup.txt").read() == "".join(t.split("_@_")[1] + "\n" for t in want["ingroup"])
    assert open(run + "_outgroup.txt").read() == "".join(t.split("_@_")[1] + "\n" for t in want["outgroup"])
    assert open(run + "_k16_s400_ingroup_nj.nwk").read() == want["ingroup_tree"]
    assert open(run + "_k16_s400_rooted_nj.nwk").read() == want["rooted_tree"]


# ---- repeatability ----
def test_repeated_and_concurrent_calls_return_the_same_bytes(gpu_ctx):
    rng = np.random.default_rng(12)
    _, fam = family(rng)
    A = [[g] for g in fam]
    big = [[bases(rng, 60000)], [bases(rng, 40000)]]
    solo = gpu_ctx.mash_distances(A, A, 21, 300, digits=None)
    solo_sk = gpu_ctx.mash_sketch(big, 21, 2000)
    out = {}

    def one():
        out["d"] = [gpu_ctx.mash_distances(A, A, 21, 300, digits=None) for _ in range(3)]

    def two():
        out["s"] = [gpu_ctx.mash_sketch(big, 21, 2000) for _ in range(3)]
    threads = [threading.Thread(target=one), threading.Thread(target=two)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for d in out["d"]:
        assert all(d[key].tobytes() == solo[key].tobytes() for key in solo)
    for sk in out["s"]:
        assert all(a.tobytes() == b.tobytes() for a, b in zip(sk, solo_sk))
    assert (solo["common"] == solo["common"].T).all() and (np.diag(solo["distance"]) == 0).all()


def test_neighbor_masher_mirror_on_the_device(gpu_ctx):
    ingroup, pool = masher_family()
    nm = tree_builder.NeighborMasher(gpu_ctx)
    nm.setMashKmerLength(16); nm.setMashSketchSize(400); nm.setExpandedIngroupSize(6); nm.setOutgroupCount(2)
    nm.setIngroupGenomes(ingroup); nm.setOutgroupGenomes(pool)
    r = nm.run()
    want = gpu_ctx.neighbor_masher(ingroup, pool, k=16, s=400, expand_ingroup=6, outgroup_count=2)
    assert nm.getIngroupTaxa() == want["ingroup"] and nm.getSelectedOutgroupTaxa() == want["outgroup"]
    assert nm.getIngroupTree() == want["ingroup_tree"] and nm.getRootedTree() == want["rooted_tree"] and r["taxa"] == want["taxa"]
