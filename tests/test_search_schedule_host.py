"""pml_search2 without a device: struct layouts, argument checks, the SPR candidate enumeration the search shares with the
door pml_debug_spr_enumerate (against tests/spr_ref.py, written from the definition), and the shim's -i parsing."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from pepr_amd import _lib, engine, synth

import spr_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WINDOWS = [(1, 5), (1, 25), (6, 10), (21, 25)]


def _caterpillar(n):
    nw = "(t0:0.1,t1:0.1)"
    for i in range(2, n - 1):
        nw = "(%s:0.1,t%d:0.1)" % (nw, i)
    return "(%s,t%d:0.1);" % (nw[1:-1], n - 1)


def _trees():
    out = [("caterpillar30", _caterpillar(30))]
    for seed in (1, 2, 3):
        out.append(("random24_%d" % seed, synth.random_tree(24, np.random.default_rng(seed))[0]))
    return out


TREES = _trees()


def test_struct_layouts_match_header():
    # pml_search_opts2 = pml_search_opts (56) + six ints; step: four ints, two doubles, a pointer; trace: see peprml.h
    assert C.sizeof(_lib.SearchOpts) == 56
    assert C.sizeof(_lib.SearchOpts2) == 80
    assert C.sizeof(_lib.SearchStep) == 40
    assert C.sizeof(_lib.SearchTrace) == 48
    assert _lib.SearchOpts2.radius_mode.offset == 56 and _lib.SearchOpts2.thorough_radius_max.offset == 76
    assert _lib.SearchStep.lnl_before.offset == 16 and _lib.SearchStep.newick_after.offset == 32
    assert _lib.SearchTrace.trial_radius.offset == 8 and _lib.SearchTrace.lnl_start.offset == 24 and _lib.SearchTrace.steps.offset == 40
    hdr = open(os.path.join(ROOT, "include", "peprml.h")).read()
    assert "#define PML_SPR_RADIUS_MAX 25" in hdr and engine.SPR_RADIUS_MAX == 25


@pytest.mark.parametrize("name,nw", TREES, ids=[t[0] for t in TREES])
def test_enumeration_matches_definition(name, nw):
    t = spr_ref.UTree(nw)
    nprunes = 0
    for p, s in t.prunes():
        pruned = t.leaves_behind(s, p)
        if len(pruned) > len(t.name) - 3:
            continue
        nprunes += 1
        for rmin, rmax in WINDOWS:
            got = engine.spr_enumerate(nw, sorted(pruned), rmin, rmax)
            ref = spr_ref.candidates(t, p, s, rmin, rmax)
            assert len(got) == len(set(got)), "an edge was listed twice"
            assert set(got) == set(ref), (name, sorted(pruned), rmin, rmax)
    assert nprunes >= 3 * (len(t.name) - 2) - 8          # every (node, neighbour) but the few that leave < 3 leaves


def test_enumeration_reaches_depth_and_tips():
    nw = _caterpillar(30)
    got = engine.spr_enumerate(nw, ["t0"], 1, 25)
    assert max(d for _, d in got) == 25 and sum(1 for far, _ in got if len(far) == 1) >= 24
    deep = engine.spr_enumerate(nw, ["t0"], 21, 25)
    assert deep and all(21 <= d <= 25 for _, d in deep)
    assert set(deep) == {c for c in got if c[1] >= 21}


def test_enumeration_honours_constraints():
    name, nw = TREES[1]
    t = spr_ref.UTree(nw)
    taxa = sorted(t.name.values())
    # two constrained splits taken from the tree itself: clades of 4..8 leaves
    clades = sorted({t.leaves_behind(s, p) for p, s in t.prunes() if 4 <= len(t.leaves_behind(s, p)) <= 8}, key=sorted)[:2]
    rows = ["".join("1" if x in c else "0" for c in clades) for x in taxa]

    def compatible(X, S):
        def ok(one):
            zero = frozenset(taxa) - one
            return not (X & one) or not (X & zero) or one <= X or zero <= X
        return all(ok(c) for c in clades)
    dropped = 0
    for p, s in t.prunes():
        pruned = t.leaves_behind(s, p)
        if len(pruned) > len(taxa) - 3:
            continue
        got = engine.spr_enumerate(nw, sorted(pruned), 1, 25, constraints=(taxa, rows))
        ref = spr_ref.candidates(t, p, s, 1, 25, allowed=lambda far: compatible(far | pruned, pruned))
        free = spr_ref.candidates(t, p, s, 1, 25)
        assert set(got) == set(ref)
        dropped += len(free) - len(ref)
    assert dropped > 0


def test_enumeration_argument_checks():
    L = _lib.load()
    nw = _caterpillar(8).encode()
    n, d, e = C.c_int(), C.c_void_p(), C.c_void_p()
    args = (0, 0, None, None, C.byref(n), C.byref(d), C.byref(e))
    assert L.pml_debug_spr_enumerate(nw, b"t0", 0, 5, *args) == -1
    assert L.pml_debug_spr_enumerate(nw, b"t0", 3, 2, *args) == -1
    assert L.pml_debug_spr_enumerate(None, b"t0", 1, 5, *args) == -1
    assert L.pml_debug_spr_enumerate(nw, b"t0\nt5", 1, 5, *args) == -6          # not a subtree
    assert L.pml_debug_spr_enumerate(nw, b"zz", 1, 5, *args) == -6
    assert L.pml_debug_spr_enumerate(b"((a,b),c", b"a", 1, 5, *args) == -2


def test_search2_rejects_null_context_and_outputs():
    L = _lib.load()
    o2 = _lib.SearchOpts2()
    assert L.pml_search2_batch(None, 1, None, None, None, C.byref(o2), None, None) == -1
    assert L.pml_search2(None, None, None, None, C.byref(o2), None, None) == -1
    L.pml_search_trace_free(None)
    t = _lib.SearchTrace()
    L.pml_search_trace_free(C.byref(t))          # an empty trace is fine


def _shim(*args):
    exe = os.path.join(ROOT, "bin", "raxmlHPC")
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("val", ["x", "0", "26", "-3", "7x"])
def test_shim_refuses_bad_radius_before_any_device_work(tmp_path, val):
    r = _shim("-f", "d", "-m", "PROTGAMMAWAG", "-s", str(tmp_path / "absent.phy"), "-n", "r", "-i", val)
    assert r.returncode != 0 and "-i" in r.stderr
    assert "device" not in r.stderr.lower() and "absent.phy" not in r.stderr


def test_shim_refuses_unknown_schedule(tmp_path):
    env = dict(os.environ, PEPRML_SEARCH_SCHEDULE="fast")
    exe = os.path.join(ROOT, "bin", "raxmlHPC")
    r = subprocess.run([exe, "-f", "d", "-m", "PROTGAMMAWAG", "-s", str(tmp_path / "absent.phy"), "-n", "r"], capture_output=True,
                       text=True, timeout=60, env=env)
    assert r.returncode != 0 and "PEPRML_SEARCH_SCHEDULE" in r.stderr


def test_mirror_schedule_switch():
    from pepr_amd import tree_builder
    r = tree_builder.RAxMLRunner()
    assert r.searchSchedule is None
    r.setSearchSchedule("raxml")
    assert r.searchSchedule == "raxml"
    with pytest.raises(ValueError):
        r.setSearchSchedule("thorough")
