"""pml_jackknife3 without a device: the options struct against the header, the documented seed formula, and the refusals the
pipeline mirror raises before it touches a context."""
import ctypes as C
import os
import re

import pytest

from pepr_amd import _lib, engine, tree_builder as tb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_opts3_layout_matches_header():
    hdr = open(os.path.join(ROOT, "include", "peprml.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} pml_jackknife_opts3;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [f.split() for f in body.split(";") if f.strip()]
    assert fields == [["pml_jackknife_opts2", "base2"], ["int", "full_method"], ["int", "support_method"], ["int", "parsimony_radius"], ["int", "pad"]]
    assert [n for n, _ in _lib.JackknifeOpts3._fields_] == [f[1] for f in fields]
    assert C.sizeof(_lib.JackknifeOpts3) == C.sizeof(_lib.JackknifeOpts2) + 4 * C.sizeof(C.c_int)
    assert _lib.JackknifeOpts3.full_method.offset == C.sizeof(_lib.JackknifeOpts2)
    assert re.search(r"enum \{ PML_TREE_ML = 0, PML_TREE_PARSIMONY = 1, PML_TREE_PARSIMONY_BL = 2 \};", hdr)
    assert (engine.TREE_ML, engine.TREE_PARSIMONY, engine.TREE_PARSIMONY_BL) == (0, 1, 2)


def test_parsimony_seeds_formula():
    def want(seed, idx):                       # (unsigned)(seed + idx), 0 replaced
        v = (seed + idx) % 2 ** 32
        return v if v else 0x9E3779B9
    for seed, reps in [(3, 5), (0, 4), (2 ** 32 - 1, 3), (2 ** 32 - 3, 4), (2 ** 40 + 7, 2), (2 ** 64 - 1, 2)]:
        full, reps_seeds = engine.jackknife_parsimony_seeds(seed, reps)
        assert full == want(seed, 0)
        assert reps_seeds == [want(seed, 1 + r) for r in range(reps)]
    assert engine.jackknife_parsimony_seeds(0, 1) == (0x9E3779B9, [1])
    assert engine.jackknife_parsimony_seeds(2 ** 32 - 1, 2) == (2 ** 32 - 1, [0x9E3779B9, 1])       # seed + 1 + 0 wraps to 0
    assert engine.jackknife_parsimony_seeds(3, 0) == (3, [])


def test_mirror_refuses_before_any_context(monkeypatch):
    def no_context():
        raise AssertionError("a context was asked for")
    monkeypatch.setattr(tb, "default_context", no_context)
    genes = [(["a", "b", "c"], ["AR", "AR", "AQ"])]
    with pytest.raises(ValueError, match="parsimony_bl"):
        tb.buildConcatenatedTreeWithGeneWiseJackKnifeSupport(genes, reps=1, supportTreeMethod=tb.PARSIMONY_BL)
    with pytest.raises(ValueError, match="FastTree"):
        tb.buildConcatenatedTreeWithGeneWiseJackKnifeSupport(genes, reps=1, fullTreeMethod=tb.FAST_TREE)
