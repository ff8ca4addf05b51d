"""Block trimming without a device: the published steps (gblocks_ref.procedure) against their closed form (gblocks_ref.closed_form)
and against the library's host door (pml_gblocks_flags_host: the functions the kernels compile, with sequential scans), on the
hand-worked cases and on random genes; PEPR's defaults; the refusals; the MSATrimmer mirror; the header."""
import json
import math
import os

import numpy as np
import pytest

from pepr_amd import engine, tree_builder
import gblocks_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "gblocks_cases.json")))
# ten rows, b1 = 6 < b2 = 9: class 2 = ten A; class 1 = six A (top = b1); class 0 = five A (top = b1 - 1) and five different
# residues; gap position = five '-' (exactly n / 2) and five A
HAND_ROWS = 10
HAND_PARAMS = dict(GOLD["params"], b1=6, b2=9, gaps=ref.HALF)
HAND_COLUMN = {"2": b"AAAAAAAAAA", "1": b"AAAAAACDEF", "0": b"AAAAACDEFG", "g": b"-----AAAAA"}


def hand_gene(classes):
    m = np.array([list(HAND_COLUMN[ch]) for ch in classes], dtype=np.uint8).T
    return ref.gene_of(m)


def class_lists(classes):
    return [0 if ch == "g" else int(ch) for ch in classes], [ch == "g" for ch in classes]


@pytest.mark.parametrize("case", GOLD["cases"], ids=[c["name"] for c in GOLD["cases"]])
def test_hand_worked_cases(case):
    cls, gp = class_lists(case["classes"])
    want = [ch == "1" for ch in case["kept"]]
    assert len(want) == len(cls)
    p = ref.resolve(HAND_ROWS, HAND_PARAMS)
    stages = ref.procedure(cls, gp, p)
    assert stages[-1] == want
    assert ref.closed_form(cls, gp, p) == stages
    hit = ref.steps_exercised(stages)
    if case["step"]:
        assert hit[case["step"] - 1] == case.get("fires", True), "the case does not exercise the step it names"
    else:
        assert not any(hit)
    gene = hand_gene(case["classes"])
    assert ref.classes(ref.matrix(gene), p) == (cls, gp)            # the columns realise the class string
    got = list(engine.gblocks_flags_host(gene, HAND_PARAMS))
    assert got == ref.flag_bytes(cls, gp, stages)
    assert [bool(f & ref.KEPT) for f in got] == want


def test_golden_file_covers_the_listed_steps():
    names = {c["name"] for c in GOLD["cases"]}
    assert {"run_of_b3", "run_of_b3_plus_1", "flank_without_class2", "block_of_b0_minus_1", "block_of_b0", "gap_one_side", "gap_both_sides",
            "cut_to_b4_minus_1", "everything_kept", "nothing_kept"} <= names
    assert {c["step"] for c in GOLD["cases"]} == {0, 1, 2, 3, 4, 5}


@pytest.mark.parametrize("gaps", [ref.NONE, ref.HALF, ref.ALL], ids=["none", "half", "all"])
def test_random_class_strings(gaps):
    """the procedure against the closed form on class strings drawn directly, short thresholds: every step fires often"""
    rng = np.random.default_rng(40 + gaps)
    fired = np.zeros(5, dtype=int)
    for _ in range(1500):
        L = int(rng.integers(0, 120))
        kind = rng.choice(4, L, p=[0.3, 0.25, 0.35, 0.1])              # 0, 1, 2, gap position
        runs = np.repeat(kind[::3], 3)[:L] if rng.random() < 0.5 and L else kind
        cls, gp = [0 if k == 3 else int(k) for k in runs], [bool(k == 3) for k in runs]
        p = {"b1": 6, "b2": 9, "b3": int(rng.integers(0, 5)), "b4": int(rng.integers(2, 7)), "b0": int(rng.integers(2, 7)), "gaps": gaps}
        stages = ref.procedure(cls, gp, p)
        assert ref.closed_form(cls, gp, p) == stages
        fired += ref.steps_exercised(stages)
    assert (fired > 100).all()


_GENES = {}


def random_genes():
    if not _GENES:
        rng = np.random.default_rng(7)
        _GENES["g"] = [ref.gene_of(ref.run_gene(rng, n, L)) for n, L in ((5, 300), (12, 700), (65, 400), (3, 90), (1, 40), (2, 40))]
    return _GENES["g"]


@pytest.mark.parametrize("gaps", [ref.NONE, ref.HALF, ref.ALL], ids=["none", "half", "all"])
def test_host_door_on_random_genes(gaps):
    fired, seen = np.zeros(5, dtype=int), set()
    for gene in random_genes():
        n = len(gene[0])
        # PEPR's values; short thresholds; b4 > b0, so that step 5 has work that step 4 did not make
        for params in ({"gaps": gaps}, {"gaps": gaps, "b1": n // 2 + 1, "b2": n, "b3": 2, "b4": 3, "b0": 4}, {"gaps": gaps, "b3": 4, "b4": 9, "b0": 3}):
            p = ref.resolve(n, params)
            cls, gp = ref.classes(ref.matrix(gene), p)
            stages = ref.procedure(cls, gp, p)
            assert ref.closed_form(cls, gp, p) == stages
            assert list(engine.gblocks_flags_host(gene, params)) == ref.flag_bytes(cls, gp, stages)
            fired += ref.steps_exercised(stages)
            seen |= set(cls)
    assert seen == {0, 1, 2}
    assert [bool(x) for x in fired] == [True, True, True, gaps != ref.ALL, True]       # without gap positions step 4 has nothing to do


def test_defaults():
    for n in range(1, 2001):
        d = engine.gblocks_defaults(n)
        assert d["b1"] == math.ceil(n * 0.8) and d["b2"] == max(d["b1"], 85 * n // 100), n
        assert (d["b3"], d["b4"], d["b0"], d["gaps"]) == (8, 10, 10, engine.GBLOCKS_GAPS_HALF)
        assert d == ref.defaults(n)
        assert n / 2 < d["b1"] <= d["b2"] <= n
    assert engine.gblocks_defaults(5)["b1"] == 4 and engine.gblocks_defaults(10)["b1"] == 8 and engine.gblocks_defaults(200)["b2"] == 170
    with pytest.raises(engine.PmlError) as e:
        engine.gblocks_defaults(0)
    assert e.value.code == engine.EINVAL


@pytest.mark.parametrize("params", [
    {"b1": 5}, {"b1": 4}, {"b1": 8, "b2": 7}, {"b1": 11, "b2": 11}, {"b2": 11}, {"b3": -1}, {"b4": 1}, {"b0": 1}, {"b4": -3}, {"gaps": 4}, {"gaps": -1},
], ids=lambda p: "_".join("%s=%d" % kv for kv in p.items()))
def test_refusals(params):
    gene = hand_gene("2222")                                        # ten rows: b1 must exceed 5
    with pytest.raises(ValueError):
        ref.resolve(HAND_ROWS, params)
    with pytest.raises(engine.PmlError) as e:
        engine.gblocks_flags_host(gene, params)
    assert e.value.code == engine.EINVAL


def test_bounds_that_are_fine():
    gene = hand_gene("2222")
    for params in ({"b1": 6, "b2": 6}, {"b1": 10, "b2": 10}, {"b4": 2, "b0": 2}, {"gaps": ref.ALL}):
        assert list(engine.gblocks_flags_host(gene, params)) == ref.flags(gene, params)
    empty = (["a", "b", "c"], [b"", b"", b""])
    assert len(engine.gblocks_flags_host(empty)) == 0 and ref.flags(empty) == []
    with pytest.raises(ValueError):
        engine._gblocks_params({"b6": 1})


class _RefCtx:
    """stands in for a Context: MSATrimmer.trim only calls gblocks_trim"""

    def gblocks_trim(self, genes, params=None):
        return [ref.trim(g, params) for g in genes]


def test_mirror_names_the_result():
    rng = np.random.default_rng(3)
    names, rows = ref.gene_of(ref.run_gene(rng, 6, 200))
    aln = tree_builder.SequenceAlignment(names, [r.decode() for r in rows], name="fam")
    out = tree_builder.MSATrimmer(_RefCtx()).trim(aln)
    assert out.getName() == "fam_trim" and out.getTaxa() == names and out.rows == ref.trim((names, aln.rows))["rows"]
    assert 0 < len(out.rows[0]) < 200
    assert tree_builder.MSATrimmer(_RefCtx()).trim(tree_builder.SequenceAlignment(names, aln.rows)).getName() == "null_trim"
    assert "not mirrored" not in tree_builder.MSATrimmer.__doc__


def test_documents_state_the_rule():
    hdr = open(os.path.join(ROOT, "include", "peprml.h")).read()
    for text in ("MSATrimmer.java:41-126", "UNPINNED", "counted by identity", "similarity-matrix", "85 n / 100", "pml_trim_pipeline"):
        assert text in hdr, text
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "unpinned" in text.lower() and "by identity" in text and "gblocks" in text.lower(), doc
