"""The gene homoplasy test on the device against the restatement of the Java (steps_ref.py): per-column Fitch steps and minimum steps
(k_fitch_sitesteps, k_steps_expand, k_colminsteps), the resampler (k_steps_resample, k_steps_table) through its door, the five
threshold methods, a forced HBM budget, determinism and the refusals.  All comparisons are for equality."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from pepr_amd import engine
import genesteps_harness as H
import steps_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "genesteps_cases.json")))
EPARSE, ENOMEM = -2, -4


def want_of(genes, tree):
    names, m, col_start = ref.concatenate(genes)
    steps, mins = ref.fitch_steps(ref.parse_newick(tree), names, m), ref.min_steps(m)
    return names, m, col_start, steps, mins


def check_result(r, names, col_start, steps, mins):
    assert r["names"] == names and r["ncols"] == col_start[-1] and r["col_start"].tolist() == col_start
    assert r["steps"].dtype == np.int32 and r["min_steps"].dtype == np.int32
    assert np.array_equal(r["steps"], steps)
    assert np.array_equal(r["min_steps"], mins)
    gs, gb, gr = ref.totals(col_start, steps, mins)
    assert r["gene_steps"].tolist() == gs and r["gene_beyond"].tolist() == gb
    assert r["gene_ratio"].view(np.uint32).tolist() == np.array(gr, dtype=np.float32).view(np.uint32).tolist()


@pytest.mark.parametrize("ntax", [4, 5, 64, 65])
def test_steps_and_min_steps(gpu_ctx, oracle_lib, ntax):
    golden = GOLD if ntax == 5 else None
    names, genes, planted = H.gene_set(ntax, 100 + ntax, golden)
    if golden:
        unrooted, rooted = GOLD["tree"], GOLD["tree_rooted"]
    else:
        unrooted, rooted = H.random_trees(np.random.default_rng(ntax), names)
    wn, m, col_start, steps, mins = want_of(genes, unrooted)
    assert wn == names and (steps != 0).any() and (mins != steps).any() and {0, 1} <= {int(x) for x in mins}
    before = gpu_ctx.gene_steps_stats()
    r = gpu_ctx.gene_steps(genes, unrooted)
    after = gpu_ctx.gene_steps_stats()
    check_result(r, names, col_start, steps, mins)
    for k in ("fitch_sitesteps", "steps_expand", "colminsteps"):                 # everything fits one sub-batch: one launch of each
        assert after[k + "_launches"] - before[k + "_launches"] == 1, k
    r2 = gpu_ctx.gene_steps(genes, rooted)                                       # rooted binary input is unrooted first
    for k in ("steps", "min_steps", "gene_steps", "gene_beyond", "gene_ratio"):
        assert r2[k].tobytes() == r[k].tobytes(), k
    for g, c, case in planted:
        at = col_start[g] + c
        assert bytes(m[:, at].tolist()).decode() == case["column"]
        assert (r["steps"][at], r["min_steps"][at]) == (case["steps"], case["min"]), case["column"]
    if golden:
        assert len(planted) >= 2 * 7 - 4 and {c["column"] for _, _, c in planted} == {c["column"] for c in GOLD["cases"] if not c.get("refused")}
    # the whole concatenation's parsimony length, by the CPU oracle on the concatenated text
    rows = [bytes(m[i].tolist()).decode() for i in range(len(names))]
    a = oracle_lib.Alignment(names, rows)
    assert int(r["steps"].sum()) == oracle_lib.parsimony_length(a, oracle_lib.Tree(unrooted, a))


def test_forced_budget_gives_the_same_bytes(gpu_ctx):
    names, genes, tree = H.budget_case()
    r = gpu_ctx.gene_steps(genes, tree)
    check_result(r, *[x for i, x in enumerate(want_of(genes, tree)) if i != 1])

    def child(budget):
        env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
        env.pop("PML_HBM_BUDGET_MB", None)
        if budget is not None:
            env["PML_HBM_BUDGET_MB"] = str(budget)
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "genesteps_harness.py")], env=env, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-2000:]
        return json.loads(p.stdout.splitlines()[-1])

    tight = child(1)
    n = tight["stats"]["fitch_sitesteps_launches"]
    assert tight["budget"] == "1" and n >= 2                                     # several sub-batches
    assert tight["stats"]["steps_expand_launches"] == n and tight["stats"]["colminsteps_launches"] == n
    want = H.digests(r)
    for k in want:
        assert tight[k] == want[k], k


# (columns per gene, target gene, mask): the domains U and gene lengths of the issue
RESAMPLE_CASES = [
    ([1, 1], 0, None),                             # U = 1, len 1
    ([1, 10, 6], 0, None),                         # U = 16
    ([63, 17], 0, None),                           # U = 17 < len 63: with replacement only
    ([5, 17], 0, None),                            # U = 17
    ([64, 4096], 0, None),                         # U = 4096
    ([50, 63, 4046], 1, None),                     # U = 4096, the target in the middle of the table
    ([65, 4000, 97], 0, None),                     # U = 4097
    ([4097, 300], 1, None),                        # U = 4097, len 300, the target last
    ([65, 100, 4097, 50], 0, [0, 1, 0, 0]),        # one other gene masked
    ([100, 65, 4097, 50], 1, [0, 1, 0, 0]),        # the target itself masked: it is not part of the table
    ([100, 300, 4097, 50], 1, [1, 1, 0, 1]),       # U = 4097 with the target and two others masked
]
REPS = [1, 63, 64, 65, 1000]


@pytest.mark.parametrize("case", range(len(RESAMPLE_CASES)))
def test_replicate_sums(gpu_ctx, case):
    lens, g, mask = RESAMPLE_CASES[case]
    fake = ref.fake_result(lens, 500 + case)
    cs = [int(x) for x in fake["col_start"]]
    U = len(ref.domain_columns(cs, g, mask))
    n = 0
    for statistic in (ref.RAW, ref.BEYOND_MIN, ref.MIN_RATIO):
        table = ref.table_of(statistic, fake["steps"], fake["min_steps"])
        for replace in (True, False):
            if not replace and U < lens[g]:
                continue
            for reps in (REPS[(case + n) % 5], 1000 if statistic == ref.BEYOND_MIN else REPS[(case + n + 2) % 5]):
                n += 1
                want = ref.replicate_sums(table, cs, g, replace, 0, reps, 31 + case, mask)
                got = gpu_ctx.debug_step_replicates(fake, g, statistic, replace, 0, reps, 0.5, 31 + case, mask)
                assert len(got) == reps
                if statistic == ref.MIN_RATIO:                                   # float sums: the same bits
                    assert got.astype(np.float32).view(np.uint32).tolist() == want.view(np.uint32).tolist(), (statistic, replace, reps)
                    assert np.array_equal(got, want.astype(np.float64))
                else:
                    assert got.tolist() == want.tolist(), (statistic, replace, reps)
    assert n >= 6


def test_replicate_sums_large_domain(gpu_ctx):
    """a C4-like table (a few MB) and the grid beyond one workgroup per gene in both modes"""
    fake = ref.fake_result([300, 1000000, 65], 9)
    cs = [int(x) for x in fake["col_start"]]
    for statistic, replace, g in ((ref.BEYOND_MIN, True, 0), (ref.MIN_RATIO, False, 2), (ref.RAW, False, 0)):
        want = ref.replicate_sums(ref.table_of(statistic, fake["steps"], fake["min_steps"]), cs, g, replace, 3, 257, 5)
        got = gpu_ctx.debug_step_replicates(fake, g, statistic, replace, 3, 257, 0.05, 5)
        assert np.array_equal(got, want.astype(np.float64)), (statistic, replace)


THRESHOLD_LENS = [40, 65, 300, 1, 700, 0]


@pytest.mark.parametrize("method", list(ref.JAVA_METHODS))
def test_thresholds_of_the_five_java_methods(gpu_ctx, method):
    statistic, replace, multiple, masked = ref.JAVA_METHODS[method]
    fake = ref.fake_result(THRESHOLD_LENS if multiple else [40, 65, 300, 1, 400, 0], 77)     # without the -1 rule every gene needs as many others
    cs = [int(x) for x in fake["col_start"]]
    mask = [0, 0, 1, 0, 0, 0] if masked else None
    reps, alpha, seed = 200, 0.05, 12
    want = [ref.java_threshold(method, fake["steps"], fake["min_steps"], cs, g, reps, alpha, seed, mask) for g in range(len(THRESHOLD_LENS))]
    got = gpu_ctx.step_thresholds(fake, statistic, replace, multiple, reps, alpha, seed, mask)
    assert got["threshold"].tolist() == [t for t, _ in want], method
    assert got["n_ge"].tolist() == [n for _, n in want], method
    if multiple:
        assert want[4] == (-1.0, -1) and want[0][1] >= 0                         # 700 columns: too few others
    assert any(0 < n < reps for _, n in want)


def test_determinism_and_independence_of_the_launch(gpu_ctx):
    fake = ref.fake_result([40, 65, 300, 1, 130], 78)
    for statistic, replace in ((ref.BEYOND_MIN, True), (ref.MIN_RATIO, False)):
        a = gpu_ctx.step_thresholds(fake, statistic, replace, 2, 130, 0.1, 3)
        b = gpu_ctx.step_thresholds(fake, statistic, replace, 2, 130, 0.1, 3)
        assert a["threshold"].tobytes() == b["threshold"].tobytes() and a["n_ge"].tobytes() == b["n_ge"].tobytes()
        obs = (fake["gene_steps"], fake["gene_beyond"], fake["gene_ratio"])[statistic]
        for g in range(5):                         # alone in its launch, through the door, a gene has the sums it has among the others
            if a["threshold"][g] < 0 and a["n_ge"][g] < 0:
                continue
            alone = gpu_ctx.debug_step_replicates(fake, g, statistic, replace, 2, 130, 0.1, 3)
            again = gpu_ctx.debug_step_replicates(fake, g, statistic, replace, 2, 130, 0.1, 3)
            assert alone.tobytes() == again.tobytes()
            assert np.sort(alone)[130 - 13] == a["threshold"][g] and int((alone >= float(obs[g])).sum()) == a["n_ge"][g], g
        # another gene's columns change the domain, but a seed changes the draws
        c = gpu_ctx.debug_step_replicates(fake, 0, statistic, replace, 2, 130, 0.1, 4)
        assert c.tobytes() != gpu_ctx.debug_step_replicates(fake, 0, statistic, replace, 2, 130, 0.1, 3).tobytes()


def test_refusals_and_launch_counts(gpu_ctx, monkeypatch):
    names = ["A", "B", "C", "D", "E"]
    ok = (names, ["ACA", "CCA", "-DA", "ADC", "AAA"])
    small = (names[:4], ["AC", "AD", "CC", "-A"])
    tree = GOLD["tree"]
    for bad_tree, what in (("((A,B),C,D,E);", "polytomy"), ("((A,B,C),D,E);", "polytomy"), ("((A,B),C,D);", "missing"),
                           ("((A,B),C,(D,(E,F)));", "F"), ("((A,B),C,(D,E)", "expected")):
        with pytest.raises(engine.PmlError) as e:
            gpu_ctx.gene_steps([ok, small], bad_tree)
        assert e.value.code == EPARSE and what in str(e.value), (bad_tree, str(e.value))
    gap = (names, ["A-A", "C?A", "--A", "A-C", "A?A"])
    with pytest.raises(engine.PmlError) as e:
        gpu_ctx.gene_steps([ok, gap], tree)
    assert e.value.code == EPARSE and "gene 1, column 1" in str(e.value)
    with pytest.raises(engine.PmlError) as e:
        gpu_ctx.gene_steps([(["A", "B", "A"], ["A", "C", "A"]), ok], tree)
    assert e.value.code == engine.EINVAL
    # a gene that alone exceeds the budget: 65 taxa x 3000 columns need more than 1 MiB
    big_names, big_genes, big_tree = H.budget_case()
    rng = np.random.default_rng(1)
    big = (big_names, ["".join(rng.choice(list("ACDE"), 3000)) for _ in big_names])
    monkeypatch.setenv("PML_HBM_BUDGET_MB", "1")
    with pytest.raises(engine.PmlError) as e:
        gpu_ctx.gene_steps([big_genes[0], big], big_tree)
    assert e.value.code == ENOMEM and "gene 1" in str(e.value) and "MiB" in str(e.value)
    monkeypatch.delenv("PML_HBM_BUDGET_MB")
    # the thresholds' refusals, and the counts of the resampling kernels
    before = gpu_ctx.gene_steps_stats()
    r = gpu_ctx.gene_steps([ok, small], tree)                                    # the same context goes on working
    fake = ref.fake_result([10, 29], 4)
    for kw in (dict(alpha=0.0), dict(alpha=1.5), dict(reps=0), dict(statistic=3), dict(multiple=-1), dict(replace=False, multiple=0)):
        a = dict(statistic=ref.BEYOND_MIN, replace=True, multiple=0, reps=5, alpha=0.5, seed=1)
        a.update(kw)
        with pytest.raises(engine.PmlError) as e:
            gpu_ctx.step_thresholds(fake, **a)
        assert e.value.code == engine.EINVAL, kw
        if "replace" in kw:
            assert "gene 1" in str(e.value)
    with pytest.raises(engine.PmlError) as e:
        gpu_ctx.debug_step_replicates(fake, 1, ref.BEYOND_MIN, True, 3, 5, 0.5, 1)          # under the -1 rule: no replicates
    assert e.value.code == engine.EINVAL
    t = gpu_ctx.step_thresholds(fake, ref.BEYOND_MIN, True, 2, 5, 0.5, 1)
    assert t["threshold"][1] == -1 and t["n_ge"][1] == -1 and t["threshold"][0] >= 0
    gpu_ctx.debug_step_replicates(r, 0, ref.MIN_RATIO, True, 0, 5, 0.5, 1)
    after = gpu_ctx.gene_steps_stats()
    d = {k: after[k] - before[k] for k in after if k.endswith("_launches")}
    assert d == {"fitch_sitesteps_launches": 1, "steps_expand_launches": 1, "colminsteps_launches": 1, "steps_resample_launches": 2, "steps_table_launches": 2}
