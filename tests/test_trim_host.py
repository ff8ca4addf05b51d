"""Column trimming, host side (no GPU): the hand-worked columns and random ones through pml_trim_column_flags_host (the decision
function k_colclass runs, compiled for the host) against the restatement of the Java (trim_ref.py); the Java's nested loop
against its closed form; the MSATrimmer mirror; the header."""
import json
import os
import re

import numpy as np
import pytest

from pepr_amd import _lib, engine, tree_builder
import trim_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "trim_cases.json")))
NEW_SYMBOLS = ["pml_trim_columns", "pml_trim_result_free", "pml_trim_congruence_filter", "pml_debug_column_flags",
               "pml_trim_column_flags_host", "pml_trim_stats"]
REQUIRED = ["AAAC", "AACC", "AAC-", "AAC?", "A?A?", "----", "-?-?"]


def gene_of_columns(cols):
    """columns (lists of byte values, all of one height) -> (names, rows as bytes)"""
    n = len(cols[0])
    return (["t%d" % i for i in range(n)], [bytes(c[r] for c in cols) for r in range(n)])


def test_golden_file_has_the_required_columns():
    have = {c["column"] for c in GOLD["cases"]}
    assert set(REQUIRED) <= have
    assert any(len({b for b in c["column"] if b not in "-?"}) == 3 for c in GOLD["cases"])           # a three-class column
    assert any(max(map(ord, c["column"])) >= 128 for c in GOLD["cases"])                               # bytes >= 128
    assert any(c["column"].lower() != c["column"] and c["column"].upper() != c["column"] for c in GOLD["cases"])   # mixed case
    by = {c["column"]: c["keep"] for c in GOLD["cases"]}
    assert by["AAAC"] == [0, 1, 0] and by["AACC"] == [0, 1, 1] and by["AAC-"][0] == 1


@pytest.mark.parametrize("case", GOLD["cases"], ids=[repr(c["column"]) for c in GOLD["cases"]])
def test_golden_cases(case):
    col = list(case["column"].encode("latin-1"))
    want = case["keep"][0] | case["keep"][1] << 1 | case["keep"][2] << 2 | case["all_gap"] << 3
    assert ref.flags(col) == want                                                   # the restatement
    assert list(engine.trim_column_flags_host(gene_of_columns([col]))) == [want]    # the library's decision function
    assert ref.topological_loop(col) == bool(case["keep"][2])                       # the Java's loop itself
    # as a str gene: one character is one byte
    assert list(engine.trim_column_flags_host((["t%d" % i for i in range(len(col))], list(case["column"])))) == [want]


def _random_columns(seed, count):
    rng = np.random.default_rng(seed)
    alphabet = np.frombuffer(b"AC-?a\x80\xc1\xff", dtype=np.uint8)
    cols = []
    for _ in range(count):
        n = int(rng.integers(1, 9))
        k = int(rng.integers(1, len(alphabet) + 1))                  # few distinct bytes per column: repeats are common
        cols.append((n, alphabet[rng.choice(len(alphabet), k, replace=False)][rng.integers(0, k, n)].tolist()))
    return cols


def test_random_columns_equal_the_restatement():
    cols = _random_columns(20261019, 4000)
    seen = set()
    for n in range(1, 9):
        group = [c for m, c in cols if m == n]
        got = engine.trim_column_flags_host(gene_of_columns(group))
        want = [ref.flags(c) for c in group]
        assert list(got) == want, n
        seen |= set(want)
    assert seen == {0, 2, 3, 6, 7, 8}          # every value that can occur: UNIFORM or TOPOLOGICAL imply GAP_UNIFORM, all-gap keeps nothing


def test_literal_loop_equals_the_closed_form():
    for _, col in _random_columns(7, 4000):
        assert ref.topological_loop(col) == ref.keep_topological(col), col
        assert ref.keep_gap_uniform(col) == (len({b for b in col if b != ref.GAP}) >= 2), col
        if ref.bipartitions(col) is not None:
            classes = {b for b in col if b not in (ref.GAP, ref.MISSING)}
            shown = sum(b not in (ref.GAP, ref.MISSING) for b in col)
            assert ref.keep_uniform(col) == (len(classes) >= 3 or (len(classes) == 2 and shown < len(col))), col


def test_trim_ref_on_a_gene():
    gene = (["x", "y", "z", "w"], ["AAA-C", "AAA-C", "ACC-D", "CC--D"])
    t = ref.trim(gene, ref.GAP_UNIFORM)
    assert t["kept_cols"] == [0, 1, 2, 4] and t["rows"] == ["AAAC", "AAAC", "ACCD", "CC-D"] and t["gap_or_missing"] == 5
    assert ref.trim(gene, ref.TOPOLOGICAL)["kept_cols"] == [1, 4]
    with pytest.raises(ValueError):
        ref.trim(gene, ref.UNIFORM)                                   # column 3 is all '-'
    assert ref.trim((gene[0], [r[:3] + r[4:] for r in gene[1]]), ref.UNIFORM)["kept_cols"] == [2]


def test_host_entry_refuses_bad_input():
    with pytest.raises(engine.PmlError) as e:
        engine.trim_column_flags_host(([], []))
    assert e.value.code == engine.EINVAL
    assert len(engine.trim_column_flags_host((["a"], [""]))) == 0


class _RefCtx:
    """stands in for a Context: MSATrimmer only calls trim_columns"""
    def trim_columns(self, genes, mode):
        return ref.trim_genes(genes, mode)


def test_msatrimmer_mirror_names():
    aln = tree_builder.SequenceAlignment(["x", "y", "z", "w"], ["AAAC", "AAAC", "ACCD", "CC-D"], name="fam7")
    assert aln.getName() == "fam7" and tree_builder.SequenceAlignment(["x"], ["A"]).getName() is None
    m = tree_builder.MSATrimmer(_RefCtx())
    a = m.trimUniformativeColumns(aln)
    b = m.trimUniformColumns(aln)
    c = m.trimTopologicallyUninformativeColumns(aln)
    assert all(isinstance(x, tree_builder.SequenceAlignment) and x.getTaxa() == aln.getTaxa() for x in (a, b, c))
    assert a.getName() == "fam7_ui" and b.getName() == "fam7_ui" and c.getName() is None
    assert a.rows == ["AAAC", "AAAC", "ACCD", "CC-D"] and b.rows == ["A", "A", "C", "-"] and c.rows == ["AC", "AC", "CD", "CD"]
    assert m.trimUniformColumns(tree_builder.SequenceAlignment(["x", "y"], ["AC", "AD"])).getName() == "null_ui"
    assert (engine.TRIM_UNIFORM, engine.TRIM_GAP_UNIFORM, engine.TRIM_TOPOLOGICAL) == (ref.UNIFORM, ref.GAP_UNIFORM, ref.TOPOLOGICAL)


def test_new_symbols_are_declared_listed_and_exported():
    header = open(os.path.join(ROOT, "include", "peprml.h")).read()
    L = _lib.load()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, header), s
        assert s in _lib.SYMBOLS, s
        assert hasattr(L, s), s
    assert "PML_TRIM_UNIFORM = 0, PML_TRIM_GAP_UNIFORM = 1, PML_TRIM_TOPOLOGICAL = 2" in header
    assert "PML_K_END = 14" in header                                # no new kernel-statistics slot
    for text in ("MSATrimmer.java:205-253", ":141-203", ":264-351", "gap_or_missing", "PML_EPARSE", "classes == 2"):
        assert text in header, text
