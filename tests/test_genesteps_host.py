"""The gene homoplasy test, host side (no GPU): the hand-worked columns against the restatement of the Java (steps_ref.py); the
Java's class loop against its closed form; the draw rules (permutation, both modes, masks) through pml_step_draws_host, the
functions k_steps_resample runs compiled for the host; the sampler's distribution; the refusals; the mirror; the tool on a stub
context; and genesteps_host.cpp alone under the host sanitizers."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from pepr_amd import _lib, engine, tree_builder
import steps_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "genesteps_cases.json")))
NEW_SYMBOLS = ["pml_gene_steps", "pml_gene_steps_result_free", "pml_step_thresholds", "pml_step_draws_host", "pml_debug_step_replicates",
               "pml_gene_steps_stats"]


def golden_gene(case):
    """the gene that holds one golden column: the taxa less the absent ones"""
    names = [t for t in GOLD["taxa"] if t not in case["absent"]]
    return names, [case["column"][GOLD["taxa"].index(t)] for t in names]


@pytest.mark.parametrize("case", GOLD["cases"], ids=[c["column"] for c in GOLD["cases"]])
def test_golden_cases(case):
    full = (GOLD["taxa"], ["AC"] * 5)                                 # holds every taxon, so the union is A..E
    names, m, col_start = ref.concatenate([full, golden_gene(case)])
    assert names == GOLD["taxa"] and col_start == [0, 2, 3]
    col = m[:, 2].tolist()
    assert bytes(col).decode() == case["column"]                      # an absent taxon reads '?'
    if case.get("refused"):
        assert ref.min_steps_loop(col) is None and ref.min_steps_closed(col) is None
        with pytest.raises(ValueError):
            ref.min_steps(m)
        return
    for tree in (GOLD["tree"], GOLD["tree_rooted"]):
        assert ref.fitch_steps(ref.parse_newick(tree), names, m)[2] == case["steps"]
    assert ref.min_steps_loop(col) == case["min"] == ref.min_steps_closed(col)
    assert case["beyond"] == case["steps"] - case["min"]
    assert ref.ratio_table([case["steps"]], [case["min"]])[0] == np.float32(case["ratio"])


def test_golden_file_has_the_required_columns():
    by = {c["column"]: c for c in GOLD["cases"]}
    for col, want in (("AACCC", (1, 0, 1, 1.0)), ("AAC-C", (1, 1, 0, 0.5)), ("ACACA", (2, 0, 2, 2.0)), ("ACDEF", (4, 4, 0, 0.8))):
        assert (by[col]["steps"], by[col]["min"], by[col]["beyond"], by[col]["ratio"]) == want
    assert any(set("BZX") <= set(c["column"]) for c in GOLD["cases"])
    assert any(c["absent"] for c in GOLD["cases"]) and any(c.get("refused") for c in GOLD["cases"])


def test_class_loop_equals_the_closed_form():
    rng = np.random.default_rng(20261019)
    alphabet = np.frombuffer(b"AC-?aX\x80\xff", dtype=np.uint8)
    seen = set()
    for _ in range(4000):
        n = int(rng.integers(1, 9))
        k = int(rng.integers(1, len(alphabet) + 1))
        col = alphabet[rng.choice(len(alphabet), k, replace=False)][rng.integers(0, k, n)].tolist()
        assert ref.min_steps_loop(col) == ref.min_steps_closed(col), col
        seen.add(ref.min_steps_closed(col))
    assert {None, 0, 1, 2, 3} <= seen


def test_fitch_restatement_on_a_worked_tree():
    names, m, _ = ref.concatenate([(["A", "B", "C", "D"], ["AC", "AC", "CA", "C-"])])
    assert list(ref.fitch_steps(ref.parse_newick("((A:1,B:2)90:1,C,D);"), names, m)) == [1, 1]
    assert list(ref.fitch_steps(ref.parse_newick("((A,C),(B,D));"), names, m)) == [2, 1]


def test_perm_is_a_bijection():
    K = ref.mix64(12345)
    for U in list(range(1, 301)) + [4096, 4097]:
        assert sorted(ref.perm(K + U, U, x) for x in range(U)) == list(range(U)), U
    U = (1 << 31) - 1
    got = {ref.perm(K, U, x) for x in range(20000)}
    assert len(got) == 20000 and max(got) < U
    assert ref.half_bits(1) == 1 and ref.half_bits(16) == 2 and ref.half_bits(17) == 3 and ref.half_bits(U) == 16


def test_vector_draws_equal_the_scalar_rules():
    for U, length, replace in ((1, 1, False), (17, 17, False), (4097, 65, False), (17, 63, True), (5000, 200, True)):
        u = ref.domain_indices(11, 2, 5, length, U, replace)
        for b in (0, 4):
            key = ref.key_of(11, 2, 5, b)
            want = [ref.draw_replace(key, j, U) if replace else ref.perm(ref.mix64(key), U, j) for j in range(length)]
            assert u[b].tolist() == want, (U, length, replace, b)


COL_START = [0, 50, 113, 113, 313, 4410]           # genes of 50, 63, 0, 200 and 4097 columns


@pytest.mark.parametrize("replace", [True, False])
@pytest.mark.parametrize("mask", [None, [0, 0, 0, 1, 0], [0, 1, 0, 0, 0], [1, 0, 0, 1, 0]], ids=["nomask", "mask3", "mask1", "mask03"])
def test_draws_host_equals_the_restatement(replace, mask):
    reps = 7
    for g in range(5):                              # with mask1 gene 1 is a masked target, with mask03 genes 0 and 3 are
        for rep in (0, 3, reps - 1):
            want = ref.replicate_columns(COL_START, g, rep, replace, 1, reps, 20261019, mask)
            if want is None:                        # the gene of 4097 columns: fewer others than it has columns
                assert g == 4
                with pytest.raises(engine.PmlError):
                    engine.step_draws_host(COL_START, g, rep, ref.BEYOND_MIN, replace, 1, reps, 0.5, 20261019, mask)
                continue
            got = engine.step_draws_host(COL_START, g, rep, ref.BEYOND_MIN, replace, 1, reps, 0.5, 20261019, mask)
            assert got.tolist() == want, (g, rep)
            own = range(COL_START[g], COL_START[g + 1])
            assert not any(c in own for c in want)                                       # never a column of the gene itself
            if mask is not None:
                assert not any(mask[int(np.searchsorted(COL_START, c, side="right")) - 1] for c in want)    # nor of a masked gene
            if not replace:
                assert len(set(want)) == len(want)


def test_sampler_distribution():
    """the inputs the issue names: seed 11, gene 2, 1000 replicates of 200 draws from a domain of 5000 Poisson(2) values.  The
    mean of the replicate sums has expectation 200 * mean(table) and variance var(table) * 200 / 1000 with replacement, times
    the finite-population factor (5000 - 200) / (5000 - 1) without; |z| <= 4 (a correct sampler fails with probability 6e-5)."""
    rng = np.random.default_rng(11)
    col_start = [0, 2500, 5000, 5200]               # gene 2 has 200 columns, the others 5000
    table = rng.poisson(2.0, 5200).astype(np.int32)
    dom = table[:5000].astype(np.float64)
    for replace in (True, False):
        sums = ref.replicate_sums(table, col_start, 2, replace, 0, 1000, 11).astype(np.float64)
        var = dom.var() * 200 * (1.0 if replace else (5000 - 200) / (5000 - 1.0))
        z = (sums.mean() - 200 * dom.mean()) / np.sqrt(var / 1000)
        print("replace %d: z of the mean replicate sum %.3f" % (replace, z))
        assert abs(z) <= 4.0, (replace, z)


def test_minus_one_rule_and_refusals():
    cs = [0, 10, 40]                                # gene 0: 10 columns, 30 others
    assert len(engine.step_draws_host(cs, 0, 0, ref.BEYOND_MIN, True, 3, 5, 0.5, 1)) == 10      # U == len * multiple: runs
    assert ref.replicate_columns(cs, 0, 0, True, 3, 5, 1) is not None
    cs = [0, 10, 39]
    assert ref.replicate_columns(cs, 0, 0, True, 3, 5, 1) is None                               # one less: the -1 rule
    with pytest.raises(engine.PmlError) as e:
        engine.step_draws_host(cs, 0, 0, ref.BEYOND_MIN, True, 3, 5, 0.5, 1)
    assert e.value.code == engine.EINVAL
    assert len(engine.step_draws_host(cs, 1, 0, ref.BEYOND_MIN, True, 0, 5, 0.5, 1)) == 29      # multiple 0: no such rule
    bad = [dict(alpha=0.0), dict(alpha=1.2), dict(alpha=float("nan")), dict(reps=0), dict(statistic=3), dict(multiple=-1),
           dict(gene=1, replace=False, multiple=0),                   # 29 columns, 10 others, without replacement: the Java loops for ever
           dict(col_start=[0, 5, 1 << 31]), dict(col_start=[0, 1, 2], reps=1 << 30), dict(col_start=[0, 5, 3]),
           dict(col_start=[0, 5], replace=True, multiple=0)]          # one gene: nothing to draw from
    for kw in bad:
        a = dict(col_start=cs, gene=0, rep=0, statistic=ref.BEYOND_MIN, replace=True, multiple=0, reps=5, alpha=0.5, seed=1)
        a.update(kw)
        with pytest.raises(engine.PmlError) as e:
            engine.step_draws_host(**a)
        assert e.value.code == engine.EINVAL, kw
    # k = ceil(reps * alpha) in [1, reps]: both ends are accepted
    assert len(engine.step_draws_host(cs, 0, 0, ref.RAW, True, 0, 5, 1.0, 1)) == 10
    assert len(engine.step_draws_host(cs, 0, 4, ref.RAW, True, 0, 5, 1e-9, 1)) == 10
    with pytest.raises(engine.PmlError):
        engine.step_draws_host(cs, 0, 5, ref.RAW, True, 0, 5, 0.5, 1)                           # rep outside the replicates


class _RefCtx:
    """stands in for a Context: the mirror and the tool call gene_steps and step_thresholds"""

    def __init__(self):
        self.calls = []

    def gene_steps(self, genes, newick):
        self.calls.append(("gene_steps", len(genes)))
        names, m, col_start = ref.concatenate(genes)
        steps, mins = ref.fitch_steps(ref.parse_newick(newick), names, m), ref.min_steps(m)
        gs, gb, gr = ref.totals(col_start, steps, mins)
        return {"names": names, "ncols": col_start[-1], "col_start": np.array(col_start, dtype=np.int64), "steps": steps, "min_steps": mins,
                "gene_steps": np.array(gs, dtype=np.int64), "gene_beyond": np.array(gb, dtype=np.int64), "gene_ratio": np.array(gr, dtype=np.float32)}

    def step_thresholds(self, result, statistic=ref.BEYOND_MIN, replace=True, multiple=3, reps=1000, alpha=0.05, seed=0, mask=None):
        self.calls.append(("step_thresholds", statistic, bool(replace), multiple, reps, alpha, seed, None if mask is None else list(mask)))
        cs = [int(x) for x in result["col_start"]]
        table = ref.table_of(statistic, result["steps"], result["min_steps"])
        obs = (result["gene_steps"], result["gene_beyond"], result["gene_ratio"])[statistic]
        out = [ref.threshold(table, obs[g], cs, g, replace, multiple, reps, alpha, seed, mask) for g in range(len(cs) - 1)]
        return {"threshold": np.array([t for t, _ in out]), "n_ge": np.array([n for _, n in out], dtype=np.int64)}

    def jackknife(self, genes, reps=100, seed=0, spr_radius_full=5):
        return {"newick": "((A:0.1,B:0.1)100:0.1,C:0.1,(D:0.1,E:0.1)90:0.1);", "support_trees": ["((A,B),C,(D,E));"] * reps, "lnl": -1.0, "alpha": 1.0,
                "nsites": sum(len(g[1][0]) for g in genes)}


def _genes(seed, lens, drop=()):
    rng = np.random.default_rng(seed)
    out = []
    for k, n in enumerate(lens):
        names = [t for t in "ABCDE" if (k, t) not in drop]
        out.append((names, ["".join(rng.choice(list("ACDE"), n)) for _ in names]))
    return out


def test_mirror_method_names_and_option_sets():
    genes = _genes(3, [12, 3, 40, 25], drop={(1, "E")})
    ctx = _RefCtx()
    c = tree_builder.ConcatenatedSequenceAlignment(genes, GOLD["tree"], ctx, seed=5)
    r = ctx.gene_steps(genes, GOLD["tree"])
    assert list(c.getStepsPerSite()) == list(r["steps"])
    assert c.getStepsForAlignment(2) == r["gene_steps"][2] and c.getTotalStepsBeyondMinimumForAlignment(0) == r["gene_beyond"][0]
    assert np.float32(c.getTotalStepsToMinimumRatioForAlignment(3)) == r["gene_ratio"][3]
    mask = [False, False, False, True]
    a = c.getThresholdStepsForAlignment(1, 20, 0.1)
    b = c.getThresholdStepsBeyondMinimumForAlignment(1, 20, 0.1)
    d = c.getThresholdStepsBeyondMinimumForAlignment(1, 20, 0.1, mask)
    e = c.getThresholdStepsBeyondMinimumForAlignmentOLD(1, 20, 0.1, mask)
    f = c.getThresholdStepsToMinimumRatioForAlignment(1, 20, 0.1, mask)
    cs = [int(x) for x in r["col_start"]]
    for got, method, m in ((a, "getThresholdStepsForAlignment", None), (b, "getThresholdStepsBeyondMinimumForAlignment", None),
                           (d, "getThresholdStepsBeyondMinimumForAlignment(mask)", mask), (e, "getThresholdStepsBeyondMinimumForAlignmentOLD", mask),
                           (f, "getThresholdStepsToMinimumRatioForAlignment", mask)):
        assert got == ref.java_threshold(method, r["steps"], r["min_steps"], cs, 1, 20, 0.1, 5, m)[0], method
    sets = [x[1:4] for x in ctx.calls if x[0] == "step_thresholds"]
    assert sets == [(ref.RAW, False, 0), (ref.BEYOND_MIN, False, 0), (ref.BEYOND_MIN, True, 3), (ref.BEYOND_MIN, False, 2), (ref.MIN_RATIO, False, 2)]
    # all genes in one call, cached per option set: another index costs no call
    n = len(ctx.calls)
    c.getThresholdStepsBeyondMinimumForAlignment(0, 20, 0.1, mask)
    assert len(ctx.calls) == n
    assert c.getThresholdStepsBeyondMinimumForAlignment(2, 20, 0.1, mask) == -1          # 40 columns, 15 unmasked others < 3 * 40
    assert (engine.STEPS_RAW, engine.STEPS_BEYOND_MIN, engine.STEPS_MIN_RATIO) == (ref.RAW, ref.BEYOND_MIN, ref.MIN_RATIO)


def test_tool_writes_the_steps_table(tmp_path, monkeypatch):
    genes = _genes(9, [30, 8, 50, 120])
    d = tmp_path / "aln"
    d.mkdir()
    for k, (names, rows) in enumerate(genes):
        (d / ("fam%d.fa" % k)).write_text("".join(">%s\n%s\n" % (t, r) for t, r in zip(names, rows)))
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import pepr_tree_step
    finally:
        sys.path.pop(0)
    ctx = _RefCtx()
    monkeypatch.setattr(pepr_tree_step.engine, "Context", lambda device=0: ctx)
    run = str(tmp_path / "run1")
    pepr_tree_step.main(["-run_name", run, "-alignment_dir", str(d), "-support_reps", "2", "-seed", "4", "-gene_steps", "50", "0.1"])
    lines = open(run + ".steps.tsv").read().splitlines()
    assert lines[0].split("\t") == ["gene", "columns", "steps", "beyond", "ratio", "threshold", "n_ge"]
    assert ("step_thresholds", ref.BEYOND_MIN, True, 3, 50, 0.1, 4, None) in ctx.calls   # the current Java rule
    r = ctx.gene_steps(genes, GOLD["tree"])
    cs = [int(x) for x in r["col_start"]]
    for k, line in enumerate(lines[1:]):
        f = line.split("\t")
        t, n_ge = ref.java_threshold("getThresholdStepsBeyondMinimumForAlignment(mask)", r["steps"], r["min_steps"], cs, k, 50, 0.1, 4, None)
        assert f[0] == "fam%d.fa" % k and int(f[1]) == cs[k + 1] - cs[k] and int(f[2]) == r["gene_steps"][k] and int(f[3]) == r["gene_beyond"][k]
        assert np.float32(float(f[4])) == r["gene_ratio"][k] and int(f[5]) == int(t) and int(f[6]) == n_ge
    assert int(lines[4].split("\t")[5]) == -1                         # 120 columns against 88 others
    # without the flag nothing of the kind is written or called
    ctx2 = _RefCtx()
    monkeypatch.setattr(pepr_tree_step.engine, "Context", lambda device=0: ctx2)
    pepr_tree_step.main(["-run_name", str(tmp_path / "run2"), "-alignment_dir", str(d), "-support_reps", "2"])
    assert not os.path.exists(str(tmp_path / "run2") + ".steps.tsv") and ctx2.calls == []


def test_new_symbols_are_declared_listed_and_exported():
    header = open(os.path.join(ROOT, "include", "peprml.h")).read()
    L = _lib.load()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, header), s
        assert s in _lib.SYMBOLS, s
        assert hasattr(L, s), s
    assert "PML_STEPS_RAW = 0, PML_STEPS_BEYOND_MIN = 1, PML_STEPS_MIN_RATIO = 2" in header
    assert "PML_K_END = 14" in header                                # no new kernel-statistics slot
    for text in ("ConcatenatedSequenceAlignment.java:65-425", "SequenceAlignment.java:1033", ":673-682", ":240-307", "dead code", "classes == 2"):
        assert text in header, text


def _case_file(path, cs, steps, mins, statistic, replace, multiple, reps, alpha, seed, mask):
    with open(path, "w") as f:
        f.write("%d\n%s\n%s\n%s\n%d %d %d %d %r %d\n%s\n" % (len(cs) - 1, " ".join(map(str, cs)), " ".join(map(str, steps)), " ".join(map(str, mins)),
                                                           statistic, int(replace), multiple, reps, alpha, seed,
                                                           "-1" if mask is None else " ".join(str(int(m)) for m in mask)))


def test_host_half_standalone_under_host_sanitizers(tmp_path):
    """genesteps_host.cpp is plain C++: built ALONE with a small main under AddressSanitizer and UndefinedBehaviorSanitizer and
    run as a program of its own; its totals, domains, draws and order statistics equal the restatement's"""
    exe = str(tmp_path / "genesteps_standalone")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           os.path.join(ROOT, "pepr_amd", "csrc", "genesteps_host.cpp"), os.path.join(ROOT, "tests", "genesteps_standalone", "main.cpp"), "-o", exe])
    fake = ref.fake_result([50, 17, 0, 65, 300], 3)
    cs, steps, mins = [int(x) for x in fake["col_start"]], fake["steps"], fake["min_steps"]
    obs = (fake["gene_steps"], fake["gene_beyond"], fake["gene_ratio"])
    for statistic, replace, multiple, reps, alpha, mask in [(ref.RAW, False, 1, 9, 0.3, None), (ref.BEYOND_MIN, True, 3, 64, 0.05, [0, 1, 0, 0, 0]),
                                                            (ref.BEYOND_MIN, False, 2, 65, 0.05, [0, 0, 0, 1, 0]), (ref.MIN_RATIO, False, 2, 10, 1.0, [0, 0, 0, 0, 1]),
                                                            (ref.MIN_RATIO, True, 0, 5, 0.5, None)]:
        path = str(tmp_path / "case.txt")
        _case_file(path, cs, steps, mins, statistic, replace, multiple, reps, alpha, 77, mask)
        r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
        lines = r.stdout.splitlines()
        for g in range(5):
            assert lines[g] == "totals %d %d %d %08x" % (g, fake["gene_steps"][g], fake["gene_beyond"][g], int(fake["gene_ratio"][g:g + 1].view(np.uint32)[0]))
        table = ref.table_of(statistic, steps, mins)
        draws = {(int(f[1]), int(f[2])): [int(x) for x in f[3:]] for f in (l.split() for l in lines) if f[0] == "draw"}
        stats = {int(f[1]): (float.fromhex(f[2]), int(f[3])) for f in (l.split() for l in lines) if f[0] == "stat"}
        plans = {int(f[1]): (int(f[3]), int(f[5])) for f in (l.split() for l in lines) if f[0] == "plan"}
        for g in range(5):
            want = ref.threshold(table, obs[statistic][g], cs, g, replace, multiple, reps, alpha, 77, mask)
            assert plans[g] == (0 if want[1] < 0 else 1, len(ref.domain_columns(cs, g, mask))), g
            if want[1] < 0:
                assert g not in stats
                continue
            assert stats[g] == want, (statistic, replace, g)
            for b in range(reps):
                assert draws[(g, b)] == ref.replicate_columns(cs, g, b, replace, multiple, reps, 77, mask), (g, b)
    # a refusal comes back as an error line, not a crash
    _case_file(str(tmp_path / "bad.txt"), cs, steps, mins, ref.RAW, False, 0, 5, 0.5, 1, [1, 1, 0, 1, 0])      # gene 4: 300 columns, 0 others
    r = subprocess.run([exe, str(tmp_path / "bad.txt")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "plan error -1 gene 4" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])
