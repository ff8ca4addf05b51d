"""Thin Python view of the C ABI (include/peprml.h): Context, resident Batch, one-shot calls.

PyTorch is not needed here; it is used only by bench.py / distributed.py for rank plumbing.
"""
import ctypes as C

import numpy as np

from . import _lib

KERNELS = {"pmat": 0, "newview": 1, "evaluate": 2, "sumtable": 3, "newton": 4, "reduce": 5,
           "host_build": 6, "host_wait": 7, "model": 8, "codehist": 9, "pairscore": 10, "colsplit": 11, "splitcost": 12, "treepairs": 13}
PI_RAXML_3DP, PI_WAG_FULL, PI_EMPIRICAL = 0, 1, 2      # PI_EMPIRICAL = PROTGAMMAWAGF (frequencies counted per gene)
SUPPORT_EQUAL_TAXA, SUPPORT_DECORATOR, SUPPORT_RESTRICTED = 0, 1, 2      # pml_jackknife2 / pml_support_tree_rule counting rules
RADIUS_FIXED, RADIUS_AUTO, SPR_RADIUS_MAX = 0, 1, 25       # pml_search_opts2.radius_mode, PML_SPR_RADIUS_MAX
PI_GTR = 3             # PROTGAMMAGTR: exchangeabilities estimated per gene by the optimising calls, empirical frequencies
NJ_DISTANCE, NJ_SIMILARITY = 0, 1      # pml_nj_from_matrix matrix types (TreeBuilder.DISTANCE / SIMILARITY)
NJ_TREE, NJ_TOPOLOGY = 0, 1            # getNJTreeString (lengths) / getNJTopology (the `-nj true` path)
TREE_ML, TREE_PARSIMONY, TREE_PARSIMONY_BL = 0, 1, 2      # pml_jackknife3 tree-building methods (PML_TREE_*)
TRIM_UNIFORM, TRIM_GAP_UNIFORM, TRIM_TOPOLOGICAL = 0, 1, 2     # pml_trim_columns modes (PML_TRIM_*): MSATrimmer's three filters
GBLOCKS_GAPS_NONE, GBLOCKS_GAPS_HALF, GBLOCKS_GAPS_ALL = 1, 2, 3     # pml_gblocks_params.gaps (PML_GBLOCKS_GAPS_*); 0 = PEPR's (HALF)
GB_CLASS, GB_GAP_POS, GB_SEL1, GB_SEL3, GB_SEL4, GB_KEPT = 3, 4, 16, 32, 64, 128      # the bits of a debug_gblocks_flags byte
STEPS_RAW, STEPS_BEYOND_MIN, STEPS_MIN_RATIO = 0, 1, 2     # pml_step_thresholds statistics (PML_STEPS_*)
EINVAL = -1
MODELDEV_DOUBLES = 20 + 400 + 400 + 20 + 400       # eval, U, Uinv, pi, Uinv transposed (kernels.h ModelDev)


class PmlError(RuntimeError):
    def __init__(self, code, detail=""):
        self.code = code
        msg = _lib.load().pml_strerror(code).decode()
        super().__init__("%s (%d)%s" % (msg, code, ": " + detail if detail else ""))


def _aln_struct(names, rows, keep):
    n = len(names)
    if n != len(rows):
        raise ValueError("names/rows length mismatch")
    L = len(rows[0]) if n else 0
    for r in rows:
        if len(r) != L:
            raise ValueError("alignment rows have different lengths")
    na = (C.c_char_p * n)(*[s.encode() if isinstance(s, str) else s for s in names])
    ra = (C.c_char_p * n)(*[s.encode() if isinstance(s, str) else s for s in rows])
    keep.extend([na, ra])
    return _lib.Alignment(n, L, na, ra)


def _raw_aln_struct(names, rows, keep):
    """as _aln_struct for the calls that compare bytes by identity: a str row is its latin-1 bytes (one byte per character)"""
    return _aln_struct(names, [r.encode("latin-1") if isinstance(r, str) else r for r in rows], keep)


def _gblocks_params(params):
    """None (PEPR's values) or a dict with any of b1, b2, b3, b4, b0, gaps (a missing or 0 field takes PEPR's value) -> the pointer
    argument of the pml_gblocks_* calls"""
    if params is None:
        return None
    unknown = set(params) - {"b1", "b2", "b3", "b4", "b0", "gaps"}
    if unknown:
        raise ValueError("unknown Gblocks parameters: %s" % sorted(unknown))
    return C.byref(_lib.GblocksParams(*[int(params.get(k, 0)) for k in ("b1", "b2", "b3", "b4", "b0", "gaps")]))


def _model(ncat=4, alpha=1.0, pi_mode=PI_RAXML_3DP):
    return _lib.Model(ncat, alpha, pi_mode)


def _opts(optimize_alpha=True, nni=True, spr_radius=0, epsilon=0.0, seed=0, constraints=None, keep=None):
    """constraints: (names, rows) -- FastTree-style 0/1/- matrix, one row per named taxon."""
    o = _lib.SearchOpts(int(optimize_alpha), int(nni), int(spr_radius), float(epsilon), int(seed), 0, 0, None, None)
    if constraints is not None:
        names, rows = constraints
        n = len(names)
        na = (C.c_char_p * n)(*[s.encode() for s in names])
        ra = (C.c_char_p * n)(*[s.encode() for s in rows])
        if keep is not None:
            keep.extend([na, ra])
        o.nconstraints = len(rows[0]) if n else 0
        o.constraint_ntax = n
        o.constraint_names = na
        o.constraint_rows = ra
        o._keep = (na, ra)
    return o


def constraints_from_tree(newick):
    """The 0/1 matrix FastTreeRunner.getFastTreeConstraintsForTree builds (FastTreeRunner.java:243-273):
    taxa sorted by name, one column per node of the constraint tree (1 = leaf below that node)."""
    import re
    s = newick.strip().rstrip(";")
    pos = 0
    cols = []

    def node():
        nonlocal pos
        leaves = []
        if s[pos] == "(":
            pos += 1
            while True:
                leaves += node()
                if s[pos] == ",":
                    pos += 1
                    continue
                if s[pos] == ")":
                    pos += 1
                    break
            m = re.match(r"[^,():;]*(:[-+0-9.eE]+)?", s[pos:])
            pos += len(m.group(0))
        else:
            m = re.match(r"([^,():;]*)(:[-+0-9.eE]+)?", s[pos:])
            pos += len(m.group(0))
            leaves = [m.group(1)]
        cols.append(set(leaves))
        return leaves
    taxa = sorted(node())
    rows = ["".join("1" if t in c else "0" for c in cols) for t in taxa]
    return taxa, rows


def _edge_sets(text, n):
    return [frozenset(b.split("\n")) for b in text.split("\n\n")] if n else []


def spr_enumerate(newick, pruned_leaves, rmin, rmax, constraints=None):
    """Host-only door of the SPR candidate enumeration the search uses: list of (far-side leaf set, distance) in engine order."""
    L = _lib.load()
    o = _opts(constraints=constraints)
    n, dist, edges = C.c_int(0), C.c_void_p(), C.c_void_p()
    rc = L.pml_debug_spr_enumerate(newick.encode(), "\n".join(pruned_leaves).encode(), int(rmin), int(rmax), o.nconstraints,
                                   o.constraint_ntax, o.constraint_names, o.constraint_rows, C.byref(n), C.byref(dist), C.byref(edges))
    if rc:
        raise PmlError(rc, L.pml_last_error(None).decode())
    try:
        d = C.cast(dist, C.POINTER(C.c_int))
        sets = _edge_sets(C.string_at(edges).decode(), n.value)
        return [(sets[i], d[i]) for i in range(n.value)]
    finally:
        L.pml_free(dist)
        L.pml_free(edges)


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def parse_paml(text):
    """PAML .dat text -> (190 exchangeabilities: lower triangle by rows, 20 frequencies), state order ARNDCQEGHILKMFPSTWYV"""
    L = _lib.load()
    ex, pi = np.zeros(190), np.zeros(20)
    rc = L.pml_matrix_parse_paml(text.encode() if isinstance(text, str) else text, _dp(ex), _dp(pi))
    if rc:
        raise PmlError(rc, L.pml_last_error(None).decode())
    return ex, pi


def _table_arg(table):
    """a 24 x 24 score table (None = BLOSUM62 as the reference loads it) as the int[576] the C ABI takes"""
    if table is None:
        return None
    t = np.ascontiguousarray(np.asarray(table).reshape(-1), dtype=np.int32)
    if t.size != 576:
        raise PmlError(EINVAL, "a score table has 24 x 24 entries")
    return (C.c_int * 576)(*t.tolist())


def blosum62_as_loaded():
    """Host only: the 24 x 24 table AlignmentUtilities.loadScoringMatrixFromResource("BLOSUM62") leaves (codes ARNDCQEGHILKMFPSTWYV,
    B, Z, X, gap): code Z holds the file's J line, code X the file's Z line, the gap row and column are 0."""
    t = (C.c_int * 576)()
    rc = _lib.load().pml_pairscore_table_blosum62(t)
    if rc:
        raise PmlError(rc)
    return np.array(t[:], dtype=np.int64).reshape(24, 24)


def nj_from_matrix(names, matrix, matrix_type=NJ_DISTANCE, form=NJ_TREE):
    """Host only: TreeBuilder.getNJTreeString (form NJ_TREE) or getNJTopology (NJ_TOPOLOGY) of an n x n matrix -- the Java's
    double operations in its order, so every length is the Java's bits.  Fewer than 4 names or a matrix that is not n x n:
    PmlError(EINVAL)."""
    L = _lib.load()
    m = np.ascontiguousarray(np.asarray(matrix, dtype=np.float64))
    n = len(names)
    if m.ndim != 2 or m.shape != (n, n):
        raise PmlError(EINVAL, "the matrix must be %d x %d, got shape %r" % (n, n, m.shape))
    na = (C.c_char_p * n)(*[s.encode() for s in names])
    out = C.c_void_p()
    rc = L.pml_nj_from_matrix(n, na, _dp(m), int(matrix_type), int(form), C.byref(out))
    if rc:
        raise PmlError(rc)
    try:
        return C.string_at(out).decode()
    finally:
        L.pml_free(out)


class Context:
    """One engine context = one HIP device + stream (one per rank / per GPU)."""

    def __init__(self, device=0, profile=False, arena_bytes=0):
        self.L = _lib.load()
        self.ptr = C.c_void_p()
        cfg = _lib.Config(device, int(profile), int(arena_bytes))
        rc = self.L.pml_create(C.byref(cfg), C.byref(self.ptr))
        if rc:
            raise PmlError(rc, self.L.pml_last_error(None).decode())

    def _check(self, rc):
        if rc:
            raise PmlError(rc, self.L.pml_last_error(self.ptr).decode())

    def close(self):
        if self.ptr:
            self.L.pml_destroy(self.ptr)
            self.ptr = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- one-shot, gene-batched ----
    def _oneshot(self, fn, genes, newicks, model, extra, after=()):
        keep = []
        n = len(genes)
        alns = (_lib.Alignment * n)(*[_aln_struct(g[0], g[1], keep) for g in genes])
        nw = None
        if newicks is not None:
            nw = (C.c_char_p * n)(*[(s.encode() if s is not None else None) for s in newicks])
        res = (_lib.Result * n)()
        rc = fn(self.ptr, n, alns, nw, C.byref(model), *extra, res, *after)
        out = []
        if rc == 0:
            for r in res:
                d = {"lnl": r.lnl, "alpha": r.alpha, "tree_length": r.tree_length, "npatterns": r.npatterns,
                     "nsites": r.nsites, "newick": C.string_at(r.newick).decode() if r.newick else None}
                if r.site_lnl:
                    d["site_lnl"] = np.ctypeslib.as_array(r.site_lnl, shape=(max(r.nsites, 1),))[:r.nsites].copy()
                out.append(d)
        for r in res:
            self.L.pml_result_free(C.byref(r))
        self._check(rc)
        return out

    def score(self, genes, newicks, alpha=1.0, ncat=4, pi_mode=PI_RAXML_3DP, site_lnl=False):
        """genes: list of (names, rows); newicks: list of str.  Fixed tree + lengths + alpha -> lnL."""
        return self._oneshot(self.L.pml_score_batch, genes, newicks, _model(ncat, alpha, pi_mode), (1 if site_lnl else 0,))

    def optimize(self, genes, newicks, alpha=1.0, ncat=4, pi_mode=PI_RAXML_3DP, optimize_alpha=True, epsilon=1e-4):
        o = _opts(optimize_alpha, False, 0, epsilon)
        return self._oneshot(self.L.pml_optimize_batch, genes, newicks, _model(ncat, alpha, pi_mode), (C.byref(o),))

    def search(self, genes, start_newicks=None, alpha=1.0, ncat=4, pi_mode=PI_RAXML_3DP, optimize_alpha=True,
               nni=True, spr_radius=0, epsilon=1e-3, constraints=None, seed=0):
        """seed != 0: RAxML-style randomised stepwise-addition parsimony start trees instead of NJ."""
        o = _opts(optimize_alpha, nni, spr_radius, epsilon, seed=seed, constraints=constraints)
        return self._oneshot(self.L.pml_search_batch, genes, start_newicks, _model(ncat, alpha, pi_mode), (C.byref(o),))

    def search2(self, genes, start_newicks=None, alpha=1.0, ncat=4, pi_mode=PI_RAXML_3DP, optimize_alpha=True, nni=True,
                radius="auto", radius_step=0, radius_max=0, thorough=False, thorough_top=0, thorough_radius_max=0,
                epsilon=1e-3, constraints=None, seed=0, trace=False):
        """RAxML's schedule (pml_search2_batch).  radius: "auto" = determined per gene on its start tree, or a fixed
        radius 0..25 (honoured, no clamp).  Returns the result dicts; with trace=True (results, traces), a trace being
        {"radius_chosen", "trial_radius", "trial_lnl", "lnl_start", "steps": [{"phase", "rmin", "rmax", "distance",
        "lnl_before", "lnl_after", "newick_after"}]}."""
        auto = radius == "auto"
        o2 = _lib.SearchOpts2()
        o2.base = _opts(optimize_alpha, nni, 0 if auto else int(radius), epsilon, seed=seed, constraints=constraints)
        o2.radius_mode = RADIUS_AUTO if auto else RADIUS_FIXED
        o2.radius_step, o2.radius_max = int(radius_step), int(radius_max)
        o2.thorough, o2.thorough_top, o2.thorough_radius_max = int(bool(thorough)), int(thorough_top), int(thorough_radius_max)
        n = len(genes)
        tr = (_lib.SearchTrace * n)() if trace else None
        try:
            res = self._oneshot(self.L.pml_search2_batch, genes, start_newicks, _model(ncat, alpha, pi_mode), (C.byref(o2),),
                                after=(tr,) if trace else (None,))
            if not trace:
                return res
            out = []
            for t in tr:
                steps = []
                for i in range(t.nsteps):
                    s = t.steps[i]
                    steps.append({"phase": s.phase, "rmin": s.rmin, "rmax": s.rmax, "distance": s.distance, "lnl_before": s.lnl_before,
                                  "lnl_after": s.lnl_after, "newick_after": C.string_at(s.newick_after).decode()})
                out.append({"radius_chosen": t.radius_chosen, "trial_radius": [t.trial_radius[i] for i in range(t.ntrials)],
                            "trial_lnl": [t.trial_lnl[i] for i in range(t.ntrials)], "lnl_start": t.lnl_start, "steps": steps})
            return res, out
        finally:
            if tr is not None:
                for t in tr:
                    self.L.pml_search_trace_free(C.byref(t))

    def debug_spr_scores(self, gene, newick, pruned_leaves, rmin, rmax, alpha=1.0, ncat=4, pi_mode=PI_RAXML_3DP, thorough_top=0):
        """Test door of one prune: list of (far-side leaf set, distance, lazy score, thorough) in engine order; thorough =
        (score, pendant, near half, far half) for the thorough_top best lazy scores (< 0: all), else None."""
        keep = []
        aln = _aln_struct(gene[0], gene[1], keep)
        m = _model(ncat, alpha, pi_mode)
        n, dist, edges, lazy, th = C.c_int(0), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        self._check(self.L.pml_debug_spr_scores(self.ptr, C.byref(aln), newick.encode(), C.byref(m), "\n".join(pruned_leaves).encode(),
                                                int(rmin), int(rmax), int(thorough_top), C.byref(n), C.byref(dist), C.byref(edges),
                                                C.byref(lazy), C.byref(th)))
        try:
            d = C.cast(dist, C.POINTER(C.c_int))
            z = C.cast(lazy, C.POINTER(C.c_double))
            t = C.cast(th, C.POINTER(C.c_double))
            sets = _edge_sets(C.string_at(edges).decode(), n.value)
            return [(sets[i], d[i], z[i], None if t[4 * i] != t[4 * i] else tuple(t[4 * i + q] for q in range(4))) for i in range(n.value)]
        finally:
            for q in (dist, edges, lazy, th):
                self.L.pml_free(q)

    def sh_support(self, genes, newicks, alpha=1.0, ncat=4, pi_mode=PI_RAXML_3DP, nboot=1000, seed=314159):
        """FastTree's SH-like local supports for given trees: list of dicts, "newick" carries 0-1 labels (3 decimals)."""
        return self._oneshot(self.L.pml_sh_support_batch, genes, newicks, _model(ncat, alpha, pi_mode), (int(nboot), int(seed)))

    def gamma20(self, genes, newicks, pi_mode=PI_WAG_FULL):
        """FastTree's `-gamma` step on given trees: list of {"lnl" (Gamma20), "alpha", "rescale", "newick" (lengths x rescale)}."""
        keep = []
        n = len(genes)
        alns = (_lib.Alignment * n)(*[_aln_struct(g[0], g[1], keep) for g in genes])
        nw = (C.c_char_p * n)(*[s.encode() for s in newicks])
        res = (_lib.Result * n)()
        rs = (C.c_double * n)()
        m = _model(4, 1.0, pi_mode)
        rc = self.L.pml_gamma20_batch(self.ptr, n, alns, nw, C.byref(m), res, rs)
        out = []
        if rc == 0:
            for r, s_ in zip(res, rs):
                out.append({"lnl": r.lnl, "alpha": r.alpha, "rescale": float(s_), "tree_length": r.tree_length,
                            "npatterns": r.npatterns, "newick": C.string_at(r.newick).decode()})
        for r in res:
            self.L.pml_result_free(C.byref(r))
        self._check(rc)
        return out

    def bootstrap(self, gene, reps=100, seed=1, spr_radius=5, epsilon=1e-3, alpha=1.0, ncat=4, pi_mode=PI_RAXML_3DP):
        """`raxmlHPC -f a -x seed -N reps`: best ML tree with percent supports + the replicate trees."""
        keep = []
        a = _aln_struct(gene[0], gene[1], keep)
        m = _model(ncat, alpha, pi_mode)
        res, rep = _lib.Result(), C.c_void_p()
        rc = self.L.pml_bootstrap(self.ptr, C.byref(a), C.byref(m), reps, seed, spr_radius, epsilon, C.byref(res), C.byref(rep))
        self._check(rc)
        out = {"lnl": res.lnl, "alpha": res.alpha, "tree_length": res.tree_length, "newick": C.string_at(res.newick).decode(),
               "replicates": C.string_at(rep).decode().splitlines() if rep else []}
        self.L.pml_result_free(C.byref(res))
        if rep:
            self.L.pml_free(rep)
        return out

    def bootstrap2(self, genes, reps=100, seed=1, method=TREE_ML, spr_radius=5, parsimony_radius=20, epsilon=1e-3, alpha=1.0, ncat=4,
                   pi_mode=PI_RAXML_3DP, replicate_pi_mode=None, replicate_alpha=None):
        """pml_bootstrap2: the column bootstrap of a gene set (`-f a -x seed -N reps`, `-Y -N reps`) with every replicate built on
        the device from the genes resident in HBM.  genes: list of (names, rows), possibly over different taxon subsets.
        -> bootstrap()'s dict plus "npatterns", "nsites" and "mp_lengths" (1 + reps: [0] the best tree, -1 = not a parsimony tree)."""
        keep = []
        n = len(genes)
        alns = (_lib.Alignment * n)(*[_aln_struct(g[0], g[1], keep) for g in genes])
        m = _model(ncat, alpha, pi_mode)
        rm = None
        if replicate_pi_mode is not None or replicate_alpha is not None:
            rm = _model(ncat, alpha if replicate_alpha is None else replicate_alpha, pi_mode if replicate_pi_mode is None else replicate_pi_mode)
        o = _lib.BootstrapOpts2(int(reps), int(method), int(seed) & 0xFFFFFFFFFFFFFFFF, int(spr_radius), int(parsimony_radius), float(epsilon),
                                C.pointer(rm) if rm is not None else None)
        res, rep = _lib.Result(), C.c_void_p()
        mp = (C.c_longlong * (1 + max(int(reps), 0)))()
        rc = self.L.pml_bootstrap2(self.ptr, n, alns, C.byref(m), C.byref(o), C.byref(res), C.byref(rep), mp)
        self._check(rc)
        out = {"lnl": res.lnl, "alpha": res.alpha, "tree_length": res.tree_length, "npatterns": res.npatterns, "nsites": res.nsites,
               "newick": C.string_at(res.newick).decode(), "replicates": C.string_at(rep).decode().splitlines() if rep else [],
               "mp_lengths": [int(v) for v in mp]}
        self.L.pml_result_free(C.byref(res))
        if rep:
            self.L.pml_free(rep)
        lnls = (C.c_double * max(int(reps), 1))()
        have = self.L.pml_boot_replicate_lnls(self.ptr, max(int(reps), 0), lnls)
        out["replicate_lnl"] = [float(lnls[i]) for i in range(max(have, 0))]       # ML replicates only: a parsimony tree has none
        return out

    def debug_boot_replicate(self, genes, sel=None, seed=1, rep=0, form=0):
        """Test door of the bootstrap kernels: what the device builds for replicate `rep` of the selection (None = all genes)
        -> {"names", "npat", "mpad", "idx" int32[npat], "cells" uint8 (form 0: codes) or uint32 (form 1: state sets) [ntax, mpad],
        "weights" float64 (form 0) or int32 (form 1) [mpad], "cmp", "diff" int64[ntax, ntax]}; padding included."""
        keep = []
        n = len(genes)
        alns = (_lib.Alignment * n)(*[_aln_struct(g[0], g[1], keep) for g in genes])
        nt, npat, mpad = C.c_int(), C.c_int(), C.c_int()
        ptrs = [C.c_void_p() for _ in range(6)]                     # idx, cells, weights, cmp, diff, names
        arr = (C.c_int * len(sel))(*sel) if sel is not None else None
        rc = self.L.pml_debug_boot_replicate(self.ptr, n, alns, len(sel) if sel is not None else 0, arr, int(seed) & 0xFFFFFFFFFFFFFFFF, int(rep),
                                             int(form), C.byref(nt), C.byref(npat), C.byref(mpad), *[C.byref(p) for p in ptrs])
        self._check(rc)
        t, m = nt.value, mpad.value
        cdt, wdt = (np.uint8, np.float64) if form == 0 else (np.uint32, np.int32)
        out = {"names": C.string_at(ptrs[5]).decode().splitlines(), "npat": npat.value, "mpad": m,
               "idx": np.frombuffer(C.string_at(ptrs[0], 4 * npat.value), dtype=np.int32).copy(),
               "cells": np.frombuffer(C.string_at(ptrs[1], np.dtype(cdt).itemsize * t * m), dtype=cdt).reshape(t, m).copy(),
               "weights": np.frombuffer(C.string_at(ptrs[2], np.dtype(wdt).itemsize * m), dtype=wdt).copy(),
               "cmp": np.frombuffer(C.string_at(ptrs[3], 8 * t * t), dtype=np.int64).reshape(t, t).copy(),
               "diff": np.frombuffer(C.string_at(ptrs[4], 8 * t * t), dtype=np.int64).reshape(t, t).copy()}
        for p in ptrs:
            self.L.pml_free(p)
        return out

    def boot_stats(self):
        """launches of k_boot_count, k_boot_index, k_boot_gather, k_boot_pairs on this context so far, their summed HIP-event
        times in ms (profile mode) and the host wall time of the replicate builds"""
        n, ms, wall = (C.c_longlong * 4)(), (C.c_double * 4)(), C.c_double()
        self._check(self.L.pml_boot_stats(self.ptr, n, ms, C.byref(wall)))
        keys = ("count", "index", "gather", "pairs")
        return {"launches": dict(zip(keys, (int(v) for v in n))), "ms": dict(zip(keys, (float(v) for v in ms))), "build_ms": wall.value}

    def parsimony(self, genes, seed=0, spr_radius=20):
        """`raxmlHPC -y` start trees (RAxMLRunner.java:215-251): list of {"newick" (topology only), "length"}."""
        keep = []
        n = len(genes)
        alns = (_lib.Alignment * n)(*[_aln_struct(g[0], g[1], keep) for g in genes])
        o = _lib.ParsimonyOpts(int(seed), int(spr_radius))
        res = (_lib.Result * n)()
        mp = (C.c_longlong * n)()
        rc = self.L.pml_parsimony_batch(self.ptr, n, alns, C.byref(o), res, mp)
        out = []
        if rc == 0:
            out = [{"newick": C.string_at(r.newick).decode(), "length": int(mp[i]), "npatterns": r.npatterns}
                   for i, r in enumerate(res)]
        for r in res:
            self.L.pml_result_free(C.byref(r))
        self._check(rc)
        return out

    def jackknife(self, genes, reps=100, subset_size=0, seed=0, spr_radius_full=5, epsilon=1e-3, alpha=1.0,
                  ncat=4, pi_mode=PI_RAXML_3DP, shard=(0, 1)):
        """Full tree + `reps` gene-subset support trees + support counts (PhylogenomicPipeline2.java:994-1126).
        genes: list of (names, rows), possibly over different taxon subsets."""
        keep = []
        n = len(genes)
        alns = (_lib.Alignment * n)(*[_aln_struct(g[0], g[1], keep) for g in genes])
        o = _lib.JackknifeOpts(reps, subset_size, seed, spr_radius_full, epsilon, int(shard[0]), int(shard[1]))
        m = _model(ncat, alpha, pi_mode)
        res = _lib.Result()
        sup = C.c_void_p()
        rc = self.L.pml_jackknife(self.ptr, n, alns, C.byref(m), C.byref(o), C.byref(res), C.byref(sup))
        self._check(rc)
        out = {"lnl": res.lnl, "alpha": res.alpha, "tree_length": res.tree_length, "npatterns": res.npatterns,
               "nsites": res.nsites, "newick": C.string_at(res.newick).decode() if res.newick else None,
               "support_trees": C.string_at(sup).decode().splitlines() if sup else []}
        self.L.pml_result_free(C.byref(res))
        if sup:
            self.L.pml_free(sup)
        return out

    def jackknife2(self, genes, reps=100, subset_size=0, seed=0, spr_radius_full=5, epsilon=1e-3, alpha=1.0, ncat=4,
                   pi_mode=PI_RAXML_3DP, support_pi_mode=None, support_alpha=None, support_rule=SUPPORT_EQUAL_TAXA, shard=(0, 1)):
        """jackknife() under any model code (per-gene codes too: every replicate gets its own model, its frequencies counted
        on the device), optionally another code for the support trees (support_pi_mode; None = the full tree's), and one of
        the SUPPORT_* counting rules (1 = what TreeSupportDecorator.addSupportValues gives on the returned strings)."""
        keep = []
        n = len(genes)
        alns = (_lib.Alignment * n)(*[_aln_struct(g[0], g[1], keep) for g in genes])
        m = _model(ncat, alpha, pi_mode)
        sm = None
        if support_pi_mode is not None or support_alpha is not None:
            sm = _model(ncat, alpha if support_alpha is None else support_alpha, pi_mode if support_pi_mode is None else support_pi_mode)
        o = _lib.JackknifeOpts2(_lib.JackknifeOpts(reps, subset_size, seed, spr_radius_full, epsilon, int(shard[0]), int(shard[1])),
                                C.pointer(sm) if sm is not None else None, int(support_rule))
        res = _lib.Result()
        sup = C.c_void_p()
        rc = self.L.pml_jackknife2(self.ptr, n, alns, C.byref(m), C.byref(o), C.byref(res), C.byref(sup))
        self._check(rc)
        out = {"lnl": res.lnl, "alpha": res.alpha, "tree_length": res.tree_length, "npatterns": res.npatterns,
               "nsites": res.nsites, "newick": C.string_at(res.newick).decode() if res.newick else None,
               "support_trees": C.string_at(sup).decode().splitlines() if sup else []}
        self.L.pml_result_free(C.byref(res))
        if sup:
            self.L.pml_free(sup)
        return out

    def jackknife3(self, genes, reps=100, subset_size=0, seed=0, spr_radius_full=5, epsilon=1e-3, alpha=1.0, ncat=4,
                   pi_mode=PI_RAXML_3DP, support_pi_mode=None, support_alpha=None, support_rule=SUPPORT_EQUAL_TAXA, shard=(0, 1),
                   full_method=TREE_ML, support_method=TREE_ML, parsimony_radius=20):
        """jackknife2() with a tree-building method for the full tree (TREE_ML, TREE_PARSIMONY, TREE_PARSIMONY_BL) and for the
        support trees (TREE_ML, TREE_PARSIMONY): parsimony trees are built from the genes resident in HBM (k_fitch_tips) and
        come back topology only.  -> jackknife2's dict plus "mp_lengths": 1 + reps Fitch lengths, [0] the full tree, [1 + r]
        replicate r of jackknife_draw's list; -1 = not a parsimony tree, or not built on this rank."""
        keep = []
        n = len(genes)
        alns = (_lib.Alignment * n)(*[_aln_struct(g[0], g[1], keep) for g in genes])
        m = _model(ncat, alpha, pi_mode)
        sm = None
        if support_pi_mode is not None or support_alpha is not None:
            sm = _model(ncat, alpha if support_alpha is None else support_alpha, pi_mode if support_pi_mode is None else support_pi_mode)
        o2 = _lib.JackknifeOpts2(_lib.JackknifeOpts(reps, subset_size, seed, spr_radius_full, epsilon, int(shard[0]), int(shard[1])),
                                 C.pointer(sm) if sm is not None else None, int(support_rule))
        o = _lib.JackknifeOpts3(o2, int(full_method), int(support_method), int(parsimony_radius), 0)
        res = _lib.Result()
        sup = C.c_void_p()
        mp = (C.c_longlong * (1 + max(reps, 0)))()
        rc = self.L.pml_jackknife3(self.ptr, n, alns, C.byref(m), C.byref(o), C.byref(res), C.byref(sup), mp)
        self._check(rc)
        out = {"lnl": res.lnl, "alpha": res.alpha, "tree_length": res.tree_length, "npatterns": res.npatterns,
               "nsites": res.nsites, "newick": C.string_at(res.newick).decode() if res.newick else None,
               "support_trees": C.string_at(sup).decode().splitlines() if sup else [], "mp_lengths": [int(v) for v in mp]}
        self.L.pml_result_free(C.byref(res))
        if sup:
            self.L.pml_free(sup)
        return out

    def fitch_stats(self):
        """k_fitch_tips and k_fitch launches on this context so far"""
        a, b = C.c_longlong(), C.c_longlong()
        self._check(self.L.pml_fitch_stats(self.ptr, C.byref(a), C.byref(b)))
        return {"tips_launches": a.value, "fitch_launches": b.value}

    def debug_fitch_tips(self, genes, sel=None):
        """Test hook for k_fitch_tips: the Fitch tip vectors it writes for the gene selection, read back, padding included
        -> (names, masks uint32[ntax, mpad], weights int32[mpad], npat)."""
        keep = []
        n = len(genes)
        alns = (_lib.Alignment * n)(*[_aln_struct(g[0], g[1], keep) for g in genes])
        nt, npat, mpad = C.c_int(), C.c_int(), C.c_int()
        masks, w, names = C.c_void_p(), C.c_void_p(), C.c_void_p()
        arr = (C.c_int * len(sel))(*sel) if sel is not None else None
        rc = self.L.pml_debug_fitch_tips(self.ptr, n, alns, len(sel) if sel is not None else 0, arr, C.byref(nt), C.byref(npat),
                                         C.byref(mpad), C.byref(masks), C.byref(w), C.byref(names))
        self._check(rc)
        mm = np.frombuffer(C.string_at(masks, 4 * nt.value * mpad.value), dtype=np.uint32).reshape(nt.value, mpad.value).copy()
        wv = np.frombuffer(C.string_at(w, 4 * mpad.value), dtype=np.int32).copy()
        nm = C.string_at(names).decode().splitlines()
        for p in (masks, w, names):
            self.L.pml_free(p)
        return nm, mm, wv, npat.value

    # ---- the reference's `nj` method: BLOSUM62 pair scores on the device (k_pairscore), TreeBuilder's NJ on the host ----
    def pairwise_scores(self, gene, table=None):
        """SequenceAlignment.getPairwiseScores: float64[ntax, ntax], S[i][j] = -1 + sum_k table[c_i(k)][c_j(k)]; table None =
        BLOSUM62 as the reference loads it.  A byte outside the 24 codes is refused (PML_EPARSE)."""
        keep = []
        a = _aln_struct(gene[0], gene[1], keep)
        out = np.zeros((a.ntax, a.ntax))
        self._check(self.L.pml_pairwise_scores(self.ptr, C.byref(a), _table_arg(table), _dp(out)))
        return out

    def debug_pairscores(self, gene, table=None, chunk_sites=0):
        """Test hook of k_pairscore: the raw integer sums (no -1) with chunk_sites sites per workgroup (0 = default)."""
        keep = []
        a = _aln_struct(gene[0], gene[1], keep)
        out = np.zeros((a.ntax, a.ntax), dtype=np.int64)
        self._check(self.L.pml_debug_pairscores(self.ptr, C.byref(a), _table_arg(table), int(chunk_sites),
                                                out.ctypes.data_as(C.POINTER(C.c_longlong))))
        return out

    def nj_tree(self, gene, table=None, form=NJ_TREE):
        """PhylogeneticTreeBuilder's `nj` method (NJ_TREE) or buildConcatenatedNeighborJoiningTree (NJ_TOPOLOGY) of one alignment."""
        keep = []
        a = _aln_struct(gene[0], gene[1], keep)
        out = C.c_void_p()
        self._check(self.L.pml_nj_tree(self.ptr, C.byref(a), _table_arg(table), int(form), C.byref(out)))
        try:
            return C.string_at(out).decode()
        finally:
            self.L.pml_free(out)

    def nj_replicates(self, genes, sel=None, table=None, form=NJ_TREE, scores=False):
        """One NJ tree per gene selection (sel: equally long lists of gene indices; None = one replicate of all genes) on the
        concatenation's sorted taxon union; every gene is scored once.  -> list of Newick strings, or with scores=True
        (trees, [float64[nu, nu] per replicate])."""
        keep = []
        n = len(genes)
        alns = (_lib.Alignment * n)(*[_aln_struct(g[0], g[1], keep) for g in genes])
        nrep, k, arr = 1, 0, None
        if sel is not None:
            nrep, k = len(sel), len(sel[0]) if len(sel) else 0
            if any(len(s) != k for s in sel):
                raise PmlError(EINVAL, "the selections must be equally long")
            arr = (C.c_int * (nrep * k))(*[g for s in sel for g in s])
        txt, sc, nt = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self._check(self.L.pml_nj_replicates(self.ptr, n, alns, nrep, k, arr, _table_arg(table), int(form), C.byref(txt),
                                             C.byref(sc) if scores else None, C.byref(nt)))
        try:
            trees = C.string_at(txt).decode().splitlines()
            if not scores:
                return trees
            nu = C.cast(nt, C.POINTER(C.c_int))[:nrep]
            flat = np.frombuffer(C.string_at(sc, 8 * sum(x * x for x in nu)), dtype=np.float64)
            mats, o = [], 0
            for x in nu:
                mats.append(flat[o:o + x * x].reshape(x, x).copy())
                o += x * x
            return trees, mats
        finally:
            for p in (txt, sc, nt):
                if p:
                    self.L.pml_free(p)

    def nj_jackknife(self, genes, reps=100, subset_size=0, seed=0, table=None, support_rule=SUPPORT_DECORATOR):
        """The gene-wise jackknife with NJ trees throughout (`-full_tree_method nj -support_tree_method nj`): the NJ tree of
        all genes with, behind the ')' of every inner node, the number of the `reps` NJ support trees (subsets of
        jackknife_draw(ngenes, reps, subset_size, seed)) that support it under support_rule -> {"newick", "support_trees"}."""
        keep = []
        n = len(genes)
        alns = (_lib.Alignment * n)(*[_aln_struct(g[0], g[1], keep) for g in genes])
        o = _lib.JackknifeOpts(reps, subset_size, seed, 0, 0.0, 0, 1)
        main, sup = C.c_void_p(), C.c_void_p()
        self._check(self.L.pml_nj_jackknife(self.ptr, n, alns, C.byref(o), _table_arg(table), int(support_rule), C.byref(main), C.byref(sup)))
        try:
            return {"newick": C.string_at(main).decode(), "support_trees": C.string_at(sup).decode().splitlines() if sup else []}
        finally:
            for p in (main, sup):
                if p:
                    self.L.pml_free(p)

    # ---- the reference's `-congruence_filter`: column splits, their counts and the genes' conflict costs on the device ----
    def _congruence_result(self, res):
        n, w, g, k = res.ntax, res.words, res.ngenes, res.nkept
        names = [res.names[i].decode() for i in range(n)]
        kept = []
        for j in range(k):
            bits = 0
            for x in range(w):
                bits |= res.kept_words[j * w + x] << (64 * x)
            kept.append((frozenset(names[i] for i in range(n) if bits >> i & 1), res.kept_count[j], res.kept_cost[j]))
        return {"names": names, "n": n, "cutoff": res.cutoff, "kept_splits": kept,
                "kept_words": np.array(res.kept_words[:k * w], dtype=np.uint64).reshape(k, w),
                "cost_sum": list(res.cost_sum[:g]), "mean_cost": list(res.mean_cost[:g]), "nsplits": list(res.nsplits[:g]),
                "nrecords": res.nrecords, "ndistinct": res.ndistinct}

    def congruence_costs(self, genes, hash_mask=None):
        """Rules 1 to 6 of the congruence filter (include/peprml.h): per gene cost_sum, mean_cost and the number of distinct
        splits; n, the sorted names, the cutoff and the kept splits as (set of names, count, cost), ascending as n-bit integers.
        hash_mask is a test door: it is ANDed onto every hash value (0: every key probes from slot 0)."""
        keep = []
        n = len(genes)
        alns = (_lib.Alignment * n)(*[_aln_struct(g[0], g[1], keep) for g in genes])
        o = None if hash_mask is None else C.byref(_lib.CongruenceOpts(1, int(hash_mask)))
        res = _lib.CongruenceResult()
        self._check(self.L.pml_congruence_costs(self.ptr, n, alns, o, C.byref(res)))
        try:
            return self._congruence_result(res)
        finally:
            self.L.pml_congruence_result_free(C.byref(res))

    def congruence_filter(self, genes, trim_percent=0.1):
        """PhylogenomicPipeline2.filterForCongruence: congruence_costs plus the selection -> {"keep": [bool per gene], "idx",
        "max_cost", "mean_cost", "cost_sum", "cutoff", "kept_splits", ...}"""
        keep = []
        n = len(genes)
        alns = (_lib.Alignment * n)(*[_aln_struct(g[0], g[1], keep) for g in genes])
        res = _lib.CongruenceResult()
        flags = (C.c_int * n)()
        self._check(self.L.pml_congruence_filter(self.ptr, n, alns, float(trim_percent), flags, C.byref(res)))
        try:
            out = self._congruence_result(res)
        finally:
            self.L.pml_congruence_result_free(C.byref(res))
        out.update(congruence_select(out["mean_cost"], trim_percent))          # idx and max_cost
        out["keep"] = [bool(f) for f in flags]
        return out

    # ---- the reference's `-uniform_trim` and MSATrimmer's sibling filters (include/peprml.h pml_trim_columns) ----
    def _trim_result(self, res, genes):
        out = []
        for g in range(res.ngenes):
            nk = res.nkept[g]
            rows = [C.string_at(res.rows[g][i], nk) for i in range(res.ntax[g])]
            if genes[g][1] and isinstance(genes[g][1][0], str):
                rows = [r.decode("latin-1") for r in rows]
            out.append({"names": list(genes[g][0]), "rows": rows, "ncols": res.ncols[g], "nkept": nk,
                        "kept_cols": [res.kept_cols[g][j] for j in range(nk)], "gap_or_missing": res.gap_or_missing[g]})
        return out

    def trim_columns(self, genes, mode=TRIM_UNIFORM):
        """MSATrimmer's column filters on the device -> per gene {"names", "rows" (the trimmed rows, str or bytes as given),
        "ncols", "nkept", "kept_cols", "gap_or_missing"}.  mode: TRIM_UNIFORM (what -uniform_trim runs), TRIM_GAP_UNIFORM,
        TRIM_TOPOLOGICAL.  Bytes are compared by identity; a str row stands for its latin-1 bytes."""
        keep = []
        n = len(genes)
        alns = (_lib.Alignment * n)(*[_raw_aln_struct(g[0], g[1], keep) for g in genes])
        res = _lib.TrimResult()
        self._check(self.L.pml_trim_columns(self.ptr, n, alns, int(mode), C.byref(res)))
        try:
            return self._trim_result(res, genes)
        finally:
            self.L.pml_trim_result_free(C.byref(res))

    def trim_congruence_filter(self, genes, mode=TRIM_UNIFORM, trim_percent=0.1):
        """`-uniform_trim -congruence_filter` in one resident call (one upload): -> congruence_filter's dict on the trimmed genes,
        plus "trimmed": trim_columns' list"""
        keep = []
        n = len(genes)
        alns = (_lib.Alignment * n)(*[_raw_aln_struct(g[0], g[1], keep) for g in genes])
        tres, res = _lib.TrimResult(), _lib.CongruenceResult()
        flags = (C.c_int * n)()
        self._check(self.L.pml_trim_congruence_filter(self.ptr, n, alns, int(mode), float(trim_percent), flags, C.byref(tres), C.byref(res)))
        try:
            out = self._congruence_result(res)
            out["trimmed"] = self._trim_result(tres, genes)
        finally:
            self.L.pml_congruence_result_free(C.byref(res))
            self.L.pml_trim_result_free(C.byref(tres))
        out.update(congruence_select(out["mean_cost"], trim_percent))          # idx and max_cost
        out["keep"] = [bool(f) for f in flags]
        return out

    def debug_column_flags(self, gene):
        """Test door of k_colclass: one byte per column as the kernel wrote it (bits 0 to 2: kept under the three modes; bit 3:
        only '-' / '?') -> uint8 array"""
        keep = []
        a = _raw_aln_struct(gene[0], gene[1], keep)
        out = np.zeros(max(a.nsites, 1), dtype=np.uint8)
        self._check(self.L.pml_debug_column_flags(self.ptr, C.byref(a), out.ctypes.data_as(C.POINTER(C.c_ubyte))))
        return out[:a.nsites]

    def trim_stats(self):
        """k_colclass / k_colgather launches on this context so far and (profile mode) the summed HIP-event times in ms of the
        two kernels and of the host-to-device copies of the genes"""
        a, b, ms = C.c_longlong(), C.c_longlong(), (C.c_double * 3)()
        self._check(self.L.pml_trim_stats(self.ptr, C.byref(a), C.byref(b), ms))
        return {"class_launches": a.value, "gather_launches": b.value, "class_ms": ms[0], "gather_ms": ms[1], "upload_ms": ms[2]}

    # ---- the reference's `-gblocks_trim` (include/peprml.h pml_gblocks_trim) and the trimming stages as one call ----
    def gblocks_trim(self, genes, params=None):
        """MSATrimmer.trim's block selection on the device -> trim_columns' list.  params: None = PEPR's (b1 = ceil(0.8 n), b3 = 8,
        half gaps), or a dict with any of b1, b2, b3, b4, b0, gaps.  The rule is the published one; parity with the Gblocks
        binary is unpinned (include/peprml.h)."""
        keep = []
        n = len(genes)
        alns = (_lib.Alignment * n)(*[_raw_aln_struct(g[0], g[1], keep) for g in genes])
        res = _lib.TrimResult()
        self._check(self.L.pml_gblocks_trim(self.ptr, n, alns, _gblocks_params(params), C.byref(res)))
        try:
            return self._trim_result(res, genes)
        finally:
            self.L.pml_trim_result_free(C.byref(res))

    def trim_pipeline(self, genes, gblocks=True, gblocks_params=None, mode=None, trim_percent=0):
        """The trimming stages in the reference's order in one resident call (one upload): Gblocks (gblocks), then the column
        filter (mode: None = none, or TRIM_*), then the congruence filter (trim_percent: 0 = none) -> {"gblocks": gblocks_trim's
        list, "trimmed": trim_columns' list on the Gblocks stage's genes, plus congruence_filter's keys}, each only for a
        stage that ran"""
        keep = []
        n = len(genes)
        alns = (_lib.Alignment * n)(*[_raw_aln_struct(g[0], g[1], keep) for g in genes])
        gres, tres, res = _lib.TrimResult(), _lib.TrimResult(), _lib.CongruenceResult()
        flags = (C.c_int * n)()
        self._check(self.L.pml_trim_pipeline(self.ptr, n, alns, _gblocks_params(gblocks_params), int(bool(gblocks)), -1 if mode is None else int(mode),
                                             float(trim_percent), flags, C.byref(gres), C.byref(tres), C.byref(res)))
        try:
            out = {}
            if trim_percent > 0:
                out = self._congruence_result(res)
                out.update(congruence_select(out["mean_cost"], trim_percent))          # idx and max_cost
                out["keep"] = [bool(f) for f in flags]
            if gblocks:
                out["gblocks"] = self._trim_result(gres, genes)
            if mode is not None:
                out["trimmed"] = self._trim_result(tres, genes)
        finally:
            self.L.pml_congruence_result_free(C.byref(res))
            self.L.pml_trim_result_free(C.byref(gres))
            self.L.pml_trim_result_free(C.byref(tres))
        return out

    def debug_gblocks_flags(self, gene, params=None):
        """Test door of k_gbclass and k_gbselect: one byte per column as the kernels wrote it (bits 0-1: class; bit 2: gap
        position; bits 4 to 7: selected after step 1, after steps 2 and 3, after step 4, kept) -> uint8 array"""
        keep = []
        a = _raw_aln_struct(gene[0], gene[1], keep)
        out = np.zeros(max(a.nsites, 1), dtype=np.uint8)
        self._check(self.L.pml_debug_gblocks_flags(self.ptr, C.byref(a), _gblocks_params(params), out.ctypes.data_as(C.POINTER(C.c_ubyte))))
        return out[:a.nsites]

    def gblocks_stats(self):
        """k_gbclass / k_gbselect launches on this context so far and (profile mode) the summed HIP-event times in ms of the two
        kernels and of the host-to-device copies; the gather counts in trim_stats"""
        a, b, ms = C.c_longlong(), C.c_longlong(), (C.c_double * 3)()
        self._check(self.L.pml_gblocks_stats(self.ptr, C.byref(a), C.byref(b), ms))
        return {"class_launches": a.value, "select_launches": b.value, "class_ms": ms[0], "select_ms": ms[1], "upload_ms": ms[2]}

    # ---- NeighborMasher: MinHash sketches, Mash distances, selection and NJ (include/peprml.h; parity with mash is unpinned) ----
    def mash_sketch(self, genomes, k=21, s=100000):
        """Genomes (each a list of records, bytes or str) -> a list of uint64 arrays: every genome's sketch, the ascending
        min(s, D) smallest distinct values.  They can be kept and handed to mash_dist later."""
        keep = []
        n = len(genomes)
        out = np.zeros((n, s), dtype=np.uint64)
        lens = (C.c_int * n)()
        self._check(self.L.pml_mash_sketch(self.ptr, n, _genome_array(genomes, keep), int(k), int(s), _ulp(out), lens))
        return [out[g, :lens[g]].copy() for g in range(n)]

    def mash_dist(self, sketches_a, sketches_b, k=21, s=100000, digits=6):
        """Every pair of two lists of sketches -> {"common", "denom" int32[na][nb], "distance" float64[na][nb]}.  digits: 6 = the
        distance as NeighborMasher reads it from mash's text, None = the double."""
        na, nb = len(sketches_a), len(sketches_b)
        a, la = _sketch_rows(sketches_a, s)
        b, lb = _sketch_rows(sketches_b, s)
        common, denom, dist = np.zeros((na, nb), dtype=np.int32), np.zeros((na, nb), dtype=np.int32), np.zeros((na, nb))
        ip = C.POINTER(C.c_int)
        self._check(self.L.pml_mash_dist(self.ptr, na, _ulp(a), la.ctypes.data_as(ip), nb, _ulp(b), lb.ctypes.data_as(ip), int(k), int(s), int(digits or 0),
                                         common.ctypes.data_as(ip), denom.ctypes.data_as(ip), _dp(dist)))
        return {"common": common, "denom": denom, "distance": dist}

    def mash_distances(self, genomes_a, genomes_b, k=21, s=100000, digits=6):
        """mash_dist of the genomes' sketches without the sketches leaving the device"""
        keep = []
        na, nb = len(genomes_a), len(genomes_b)
        common, denom, dist = np.zeros((na, nb), dtype=np.int32), np.zeros((na, nb), dtype=np.int32), np.zeros((na, nb))
        ip = C.POINTER(C.c_int)
        self._check(self.L.pml_mash_distances(self.ptr, na, _genome_array(genomes_a, keep), nb, _genome_array(genomes_b, keep), int(k), int(s), int(digits or 0),
                                              common.ctypes.data_as(ip), denom.ctypes.data_as(ip), _dp(dist)))
        return {"common": common, "denom": denom, "distance": dist}

    def debug_mash_hashes(self, genome, k=21):
        """Test door of k_mash_hash: one uint64 per byte of every record in order; MASH_INVALID where no valid window starts"""
        keep = []
        g = _genome_array([genome], keep)
        out = np.zeros(max(sum(len(r) for r in genome), 1), dtype=np.uint64)
        self._check(self.L.pml_debug_mash_hashes(self.ptr, g, int(k), _ulp(out)))
        return out[:sum(len(r) for r in genome)]

    def debug_mash_full_sort(self, on):
        """Test / measurement door: every cut takes everything, i.e. all values of a genome are sorted (the baseline)"""
        self._check(self.L.pml_debug_mash_full_sort(self.ptr, int(bool(on))))

    def mash_stats(self):
        """Launches of the five MinHash kernels on this context so far, (profile mode) summed HIP-event times in ms, and how many
        sub-batches were repeated with a raised cut"""
        n, ms, rep = (C.c_longlong * 5)(), (C.c_double * 4)(), C.c_longlong()
        self._check(self.L.pml_mash_stats(self.ptr, n, ms, C.byref(rep)))
        return {"hash_launches": n[0], "cut_launches": n[1], "compact_launches": n[2], "unique_launches": n[3], "pairs_launches": n[4],
                "upload_ms": ms[0], "hash_ms": ms[1], "select_ms": ms[2], "pairs_ms": ms[3], "repeats": rep.value}

    def neighbor_masher(self, ingroup, pool, k=21, s=100000, outgroup_count=3, expand_ingroup=0, ingroup_only=False, outgroup_only=False, digits=6):
        """NeighborMasher.run() as one call.  ingroup, pool: lists of (taxon name, genome).  -> {"ingroup": the final ingroup's
        names, "outgroup": the selected pool names, "ingroup_index" / "outgroup_index", "candidate_distance", "mean", "sd", "max",
        "taxa" (outgroups first), "distance", "common", "denom" (len(taxa) squared, as fed to NJ), "sketch_len", "ingroup_tree",
        "rooted_tree" (None where run() builds none; the second tree is NOT rooted: include/peprml.h)}"""
        keep = []
        ni, npool = len(ingroup), len(pool)
        names = [t[0] for t in ingroup] + [t[0] for t in pool]
        ina = (C.c_char_p * max(ni, 1))(*[t[0].encode() for t in ingroup])
        pna = (C.c_char_p * max(npool, 1))(*[t[0].encode() for t in pool])
        o = _lib.NeighborMasherOpts(ni, npool, _genome_array([t[1] for t in ingroup], keep), _genome_array([t[1] for t in pool], keep), ina, pna,
                                    int(k), int(s), int(outgroup_count), int(expand_ingroup), int(bool(ingroup_only)), int(bool(outgroup_only)), int(digits or 0))
        r = _lib.NeighborMasherResult()
        self._check(self.L.pml_neighbor_masher(self.ptr, C.byref(o), C.byref(r)))
        try:
            T = r.n_taxa
            ing, outg = [r.ingroup[i] for i in range(r.n_ingroup)], [r.outgroup[i] for i in range(r.n_outgroup)]
            arr = lambda p, dt: np.array(p[:T * T], dtype=dt).reshape(T, T)      # noqa: E731
            return {"ingroup": [names[i] for i in ing], "outgroup": [names[ni + p] for p in outg], "ingroup_index": ing, "outgroup_index": outg,
                    "candidate_distance": np.array(r.candidate_distance[:r.n_pool]) if r.candidate_distance else None,
                    "mean": r.mean, "sd": r.sd, "max": r.max, "taxa": [names[r.taxa[i]] for i in range(T)],
                    "distance": arr(r.distance, np.float64), "common": arr(r.common, np.int32), "denom": arr(r.denom, np.int32),
                    "sketch_len": [r.sketch_len[i] for i in range(ni + npool)],
                    "ingroup_tree": C.string_at(r.ingroup_tree).decode() if r.ingroup_tree else None,
                    "rooted_tree": C.string_at(r.rooted_tree).decode() if r.rooted_tree else None}
        finally:
            self.L.pml_neighbor_masher_result_free(C.byref(r))

    # ---- homolog groups: Markov clustering of the hit graph (include/peprml.h "Homolog groups") ----
    def mcl_cluster(self, n, arcs, inflation=0.0, prune_inverse=0.0, chaos_eps=0.0, max_iter=0):
        """Nodes 0 .. n-1 and arcs [(a, b, w)] -> {"clusters": lists of ascending node indices in mcl's output order, "cluster_of"
        int32[n], "iterations": the slowest component's}.  Zeros are the defaults (1.5, 10000, 1e-3, 10000)."""
        a, b, w = _arc_arrays(arcs)
        out, nc, it = np.zeros(max(n, 1), dtype=np.int32), C.c_int(), C.c_int()
        o = _lib.MclOpts(float(inflation), float(prune_inverse), float(chaos_eps), int(max_iter), 0)
        ip = C.POINTER(C.c_int)
        self._check(self.L.pml_mcl_cluster(self.ptr, int(n), a.size, a.ctypes.data_as(ip), b.ctypes.data_as(ip), _dp(w), C.byref(o), out.ctypes.data_as(ip),
                                           C.byref(nc), C.byref(it)))
        return {"clusters": _clusters_of(out[:n], nc.value), "cluster_of": out[:n].copy(), "iterations": it.value}

    def homolog_groups(self, table, score_field=11, bidirectional=False, inflation=0.0, prune_inverse=0.0, chaos_eps=0.0, max_iter=0, taxon_of=None,
                       min_taxa=0, max_taxa=2 ** 31 - 1, rep_only=False, target_ntax=0, target_min_gene=0):
        """The hit table (bytes or str) to PEPR's gene sets.  taxon_of: {label: taxon number} switches the set selection on.
        -> {"labels", "clusters" (lists of node indices, mcl's order), "lines" (mcl's output lines), "mcl_text", "kept" (cluster
        indices), "components", "iterations", "filtered_text" (the <hits>_filtered / <hits>_bidir file; None with score_field 2)}"""
        t = table.encode() if isinstance(table, str) else bytes(table)
        o = _lib.HomologGroupsOpts()
        o.table, o.table_bytes, o.score_field, o.bidirectional = t, len(t), int(score_field), int(bool(bidirectional))
        o.mcl = _lib.MclOpts(float(inflation), float(prune_inverse), float(chaos_eps), int(max_iter), 0)
        if taxon_of:
            labs = list(taxon_of)
            la = (C.c_char_p * len(labs))(*[x.encode() for x in labs])
            ta = (C.c_int * len(labs))(*[int(taxon_of[x]) for x in labs])
            o.ntaxon_labels, o.taxon_labels, o.taxon_of = len(labs), la, ta
        o.min_taxa, o.max_taxa, o.rep_only, o.target_ntax, o.target_min_gene = int(min_taxa), int(max_taxa), int(bool(rep_only)), int(target_ntax), int(target_min_gene)
        r = _lib.HomologGroupsResult()
        self._check(self.L.pml_homolog_groups(self.ptr, C.byref(o), C.byref(r)))
        try:
            labels = [r.labels[i].decode() for i in range(r.nlabels)]
            off = [r.cluster_off[k] for k in range(r.nclusters + 1)]
            clusters = [[r.members[i] for i in range(off[k], off[k + 1])] for k in range(r.nclusters)]
            text = C.string_at(r.mcl_text).decode()
            return {"labels": labels, "clusters": clusters, "lines": [ln for ln in text.split("\n") if ln], "mcl_text": text,
                    "kept": [r.kept[i] for i in range(r.nkept)], "components": r.ncomponents, "iterations": r.iterations,
                    "filtered_text": C.string_at(r.filtered_text).decode() if r.filtered_text else None}
        finally:
            self.L.pml_homolog_groups_result_free(C.byref(r))

    def debug_mcl_steps(self, matrix, nsteps=1, force_class=0, inflation=0.0, prune_inverse=0.0):
        """Test door: nsteps iterations of one column-stochastic matrix (M[i][j]) in class 0 (packed), 1 (LDS) or 2 (HBM) ->
        (the matrix, the last iteration's chaos)"""
        m = np.ascontiguousarray(matrix, dtype=np.float64)
        out, chaos = np.zeros_like(m), C.c_double()
        o = _lib.MclOpts(float(inflation), float(prune_inverse), 0.0, 0, 0)
        self._check(self.L.pml_debug_mcl_steps(self.ptr, m.shape[0], _dp(m), C.byref(o), int(nsteps), int(force_class), _dp(out), C.byref(chaos)))
        return out, chaos.value

    def mcl_stats(self):
        """Launches of the Markov clustering kernels on this context so far, sub-batches, and (profile mode) ms per stage"""
        n, ms = (C.c_longlong * 8)(), (C.c_double * 4)()
        self._check(self.L.pml_mcl_stats(self.ptr, n, ms))
        return {"fill_launches": n[0], "packed_launches": n[1], "lds_launches": n[2], "expand_launches": n[3], "inflate_launches": n[4],
                "flag_launches": n[5], "read_launches": n[6], "sub_batches": n[7],
                "upload_fill_ms": ms[0], "packed_ms": ms[1], "lds_ms": ms[2], "hbm_ms": ms[3]}

    # ---- homology search: the all-vs-each Smith-Waterman hit table (include/peprml.h "Homology search") ----
    def sw_search(self, genomes, **opts):
        """genomes: a list of genomes, each a list of (title, residues) in file order -> the hit table and its hits as
        sw_search_host returns them.  Options as there."""
        keep = []
        st, o, r = _sw_set(genomes, keep), _sw_opts(opts, keep), _lib.SwResult()
        self._check(self.L.pml_sw_search(self.ptr, C.byref(st), C.byref(o), C.byref(r)))
        return _sw_result(r)

    def debug_sw_scores(self, queries, subjects, force_class=-1, force_path=0, **opts):
        """Test door: the raw score of every (query, subject) pair, no selection -> int32[nq][ns].  force_class 0 .. 2 runs
        every query in that class."""
        keep = []
        qa = (C.c_char_p * max(len(queries), 1))(*[_sw_bytes(x) for x in queries])
        sa = (C.c_char_p * max(len(subjects), 1))(*[_sw_bytes(x) for x in subjects])
        out = np.zeros((len(queries), len(subjects)), dtype=np.int32)
        o = _sw_opts(opts, keep)
        self._check(self.L.pml_debug_sw_scores(self.ptr, len(queries), qa, len(subjects), sa, C.byref(o), int(force_class), int(force_path),
                                               out.ctypes.data_as(C.POINTER(C.c_int))))
        return out

    def msa_align(self, sets, **opts):
        """Multiple alignment of many sets in one call (include/peprml.h "Multiple alignment"): sets = a list of lists of residue
        texts.  Options: gap_open, gap_extend (0 = 11, 1), table (576 ints).  -> one {"rows" (aligned texts in input order),
        "merges" [(x, y, level, score)]} per set, as msa_align_host returns them"""
        keep = []
        sa, o = _msa_sets(sets, keep), _msa_opts(opts, keep)
        res = (_lib.MsaResult * max(len(sets), 1))()
        self._check(self.L.pml_msa_align(self.ptr, len(sets), sa, C.byref(o), res))
        return [_msa_result(res[i]) for i in range(len(sets))]

    def msa_profile_align(self, a, b, force_class=-1, **opts):
        """Two alignments (lists of equally long rows, `-` a gap) aligned as profiles: a is X, b is Y.  -> {"score", "rows" (a's
        rows, then b's), "path" (per merged column 0 both, 1 b's column only, 2 a's only), "merges"}.  force_class (test door):
        the kernel's class, -1 = by a's length"""
        keep = []
        sa, sb, o, r, sc = _msa_sets([a], keep), _msa_sets([b], keep), _msa_opts(opts, keep), _lib.MsaResult(), C.c_longlong()
        if force_class == -1:
            self._check(self.L.pml_msa_profile_align(self.ptr, sa, sb, C.byref(o), C.byref(sc), C.byref(r)))
        else:
            self._check(self.L.pml_debug_msa_profile_align(self.ptr, sa, sb, C.byref(o), int(force_class), C.byref(sc), C.byref(r)))
        out = _msa_result(r)
        out["score"] = sc.value
        return out

    def msa_stats(self):
        """{"launches": k_msa_colv, k_msa_dp, k_msa_walk, k_msa_gather launches on this context so far, "merges", "levels",
        "sub_batches", "cells", "ms": (profile mode) the four kernels' HIP-event times}"""
        n, ms = (C.c_longlong * 8)(), (C.c_double * 4)()
        self._check(self.L.pml_msa_stats(self.ptr, n, ms))
        return {"launches": [n[i] for i in range(4)], "merges": n[4], "levels": n[5], "sub_batches": n[6], "cells": n[7], "ms": [ms[i] for i in range(4)]}

    def sw_stats(self):
        """k_sw_score launches per class and work units on this context so far, the DP cells they covered, and (profile mode) ms"""
        n, cells, ms = (C.c_longlong * 4)(), C.c_longlong(), (C.c_double * 4)()
        self._check(self.L.pml_sw_stats(self.ptr, n, C.byref(cells), ms))
        return {"launches": [n[0], n[1], n[2]], "units": n[3], "cells": cells.value, "class_ms": [ms[0], ms[1], ms[2]], "upload_ms": ms[3]}

    # ---- the gene homoplasy test of ConcatenatedSequenceAlignment (include/peprml.h pml_gene_steps, pml_step_thresholds) ----
    def gene_steps(self, genes, newick):
        """Per-column Fitch steps of the concatenation of `genes` on `newick`, the least steps each column can take, and the
        Java's per-gene totals -> {"names" (the sorted union), "ncols", "col_start" int64[G + 1], "steps", "min_steps" int32[ncols],
        "gene_steps", "gene_beyond" int64[G], "gene_ratio" float32[G]}.  Bytes are compared by identity for min_steps; a str row
        stands for its latin-1 bytes."""
        keep = []
        n = len(genes)
        alns = (_lib.Alignment * n)(*[_raw_aln_struct(g[0], g[1], keep) for g in genes])
        res = _lib.GeneStepsResult()
        self._check(self.L.pml_gene_steps(self.ptr, n, alns, newick.encode() if isinstance(newick, str) else newick, C.byref(res)))
        try:
            nc, G = res.ncols, res.ngenes
            return {"names": [res.names[i].decode() for i in range(res.ntax)], "ncols": nc,
                    "col_start": np.ctypeslib.as_array(res.col_start, (G + 1,)).copy(),
                    "steps": np.ctypeslib.as_array(res.steps, (max(nc, 1),))[:nc].copy(),
                    "min_steps": np.ctypeslib.as_array(res.min_steps, (max(nc, 1),))[:nc].copy(),
                    "gene_steps": np.ctypeslib.as_array(res.gene_steps, (G,)).copy(),
                    "gene_beyond": np.ctypeslib.as_array(res.gene_beyond, (G,)).copy(),
                    "gene_ratio": np.ctypeslib.as_array(res.gene_ratio, (G,)).copy()}
        finally:
            self.L.pml_gene_steps_result_free(C.byref(res))

    def step_thresholds(self, result, statistic=STEPS_BEYOND_MIN, replace=True, multiple=3, reps=1000, alpha=0.05, seed=0, mask=None):
        """The randomisation thresholds of every gene of a gene_steps result -> {"threshold" float64[G] (-1: too few columns to
        draw from), "n_ge" int64[G]: the replicates whose sum is >= the gene's observed total}.  The defaults are the Java's
        current rule (:240-307)."""
        res, keep = _gene_steps_struct(result)
        o = _step_opts(statistic, replace, multiple, reps, alpha, seed, mask, res.ngenes, keep)
        thr, nge = np.zeros(res.ngenes, dtype=np.float64), np.zeros(res.ngenes, dtype=np.int64)
        self._check(self.L.pml_step_thresholds(self.ptr, C.byref(res), C.byref(o), _dp(thr), nge.ctypes.data_as(C.POINTER(C.c_longlong))))
        return {"threshold": thr, "n_ge": nge}

    def debug_step_replicates(self, result, gene, statistic=STEPS_BEYOND_MIN, replace=True, multiple=3, reps=1000, alpha=0.05, seed=0, mask=None):
        """Test door of k_steps_resample: the kernel's replicate sums of one gene, alone in its launch, unsorted -> float64[reps]"""
        res, keep = _gene_steps_struct(result)
        o = _step_opts(statistic, replace, multiple, reps, alpha, seed, mask, res.ngenes, keep)
        sums = np.zeros(max(int(reps), 1), dtype=np.float64)
        self._check(self.L.pml_debug_step_replicates(self.ptr, C.byref(res), C.byref(o), int(gene), _dp(sums)))
        return sums[:int(reps)]

    GENE_STEPS_KERNELS = ("fitch_sitesteps", "steps_expand", "colminsteps", "steps_resample", "steps_table")

    def gene_steps_stats(self):
        """launches of the gene-steps kernels on this context so far and (profile mode) their summed HIP-event times in ms"""
        n, ms = (C.c_longlong * 5)(), (C.c_double * 5)()
        self._check(self.L.pml_gene_steps_stats(self.ptr, n, ms))
        out = {}
        for k, name in enumerate(self.GENE_STEPS_KERNELS):
            out[name + "_launches"], out[name + "_ms"] = n[k], ms[k]
        return out

    # ---- TreeComparison's -rf / -tree_dist legs for a set of trees (include/peprml.h pml_tree_compare) ----
    TREE_COMPARE_ARRAYS = (("rf_legacy", 1, np.int32), ("rf_bipartition", 2, np.int32), ("rf_splits", 4, np.int32),
                           ("branch_dist", 8, np.float64), ("discrepant_dist", 16, np.float64))

    def _tree_compare_opts(self, window, use_lengths, want):
        bits = 0
        for name, bit, _ in self.TREE_COMPARE_ARRAYS:
            if want is None or name in want:
                bits |= bit
        if want is not None and not bits:
            raise ValueError("want names none of " + ", ".join(a[0] for a in self.TREE_COMPARE_ARRAYS))
        return _lib.TreeCompareOpts(int(window), 1 if use_lengths else 0, bits)

    def _tree_compare_result(self, res, one):
        try:
            shape = (res.ncols,) if one else (res.nrows, res.ncols)
            out = {"ntax": res.ntax, "row_blocks": res.row_blocks, "resident_bytes": res.resident_bytes, "row_bytes": res.row_bytes}
            for name, _, dt in self.TREE_COMPARE_ARRAYS:
                p = getattr(res, name)
                if p:
                    out[name] = np.ctypeslib.as_array(p, shape=(res.nrows * res.ncols,)).astype(dt).reshape(shape)
            return out
        finally:
            self.L.pml_tree_compare_result_free(C.byref(res))

    def tree_compare(self, newicks, window=0, use_lengths=True, want=None):
        """Every pair of a set of trees over one leaf set, as TreeComparison.compareAllvsAll computes it (tree 1 = the lower
        index) -> {"rf_legacy", "rf_bipartition", "rf_splits": int32 [T, T]; "branch_dist", "discrepant_dist": float64 [T, T]}.
        window = w > 0: only |i - j| <= w, the rest -1 / NaN.  want: the names of the arrays to produce (None = all)."""
        o = self._tree_compare_opts(window, use_lengths, want)
        na = (C.c_char_p * max(len(newicks), 1))(*[s.encode() for s in newicks])
        res = _lib.TreeCompareResult()
        self._check(self.L.pml_tree_compare(self.ptr, len(newicks), na, C.byref(o), C.byref(res)))
        return self._tree_compare_result(res, False)

    def tree_compare_one(self, standard, newicks, use_lengths=True, want=None):
        """TreeComparison.calculateTreeDistances: the standard tree (tree 1) against each tree -> the same arrays, shape [T]"""
        o = self._tree_compare_opts(0, use_lengths, want)
        na = (C.c_char_p * max(len(newicks), 1))(*[s.encode() for s in newicks])
        res = _lib.TreeCompareResult()
        self._check(self.L.pml_tree_compare_one(self.ptr, standard.encode(), len(newicks), na, C.byref(o), C.byref(res)))
        return self._tree_compare_result(res, True)

    def debug_tree_splits(self, newicks, use_lengths=True):
        """Test door: the split records of a tree set as the kernels see them -> {"names", "first" [T + 1], "nreal" [T], "splits"
        (ints, taxon i = bit i), "length", "length_norm", "flags", "split_id"}, records in branch order per tree"""
        na = (C.c_char_p * max(len(newicks), 1))(*[s.encode() for s in newicks])
        res = _lib.TreeSplits()
        self._check(self.L.pml_debug_tree_splits(self.ptr, len(newicks), na, 1 if use_lengths else 0, C.byref(res)))
        try:
            N, w, T = res.nrecords, res.words, res.ntrees
            words = np.array(res.split_words[:N * w], dtype=np.uint64).reshape(N, w)
            return {"names": [res.names[i].decode() for i in range(res.ntax)], "first": list(res.first[:T + 1]), "nreal": list(res.nreal[:T]),
                    "splits": [sum(int(r[x]) << (64 * x) for x in range(w)) for r in words],
                    "length": np.array(res.length[:N]), "length_norm": np.array(res.length_norm[:N]),
                    "flags": list(res.flags[:N]), "split_id": list(res.split_id[:N]), "words": w}
        finally:
            self.L.pml_tree_splits_free(C.byref(res))

    def debug_tree_pair_sums(self, newicks, pairs, use_lengths=True):
        """Test door: the raw results of chosen pairs (i <= j, tree 1 = i) -> (counts int64 [P, 7], sums float64 [P, 6]): shared,
        shared non-trivial, shared resolved, distinct / distinct non-trivial of i and of j; r, ss1, ss2 of getBranchDistance and
        of getDiscrepantBranchDistance"""
        na = (C.c_char_p * max(len(newicks), 1))(*[s.encode() for s in newicks])
        P = len(pairs)
        flat = (C.c_int * max(2 * P, 1))(*[int(x) for p in pairs for x in p])
        counts = np.zeros((P, 7), dtype=np.int64)
        sums = np.zeros((P, 6), dtype=np.float64)
        self._check(self.L.pml_debug_tree_pair_sums(self.ptr, len(newicks), na, 1 if use_lengths else 0, P, flat,
                                                    counts.ctypes.data_as(C.POINTER(C.c_longlong)), sums.ctypes.data_as(C.POINTER(C.c_double))))
        return counts, sums

    def debug_column_splits(self, gene, names_union):
        """Test hook of k_colsplits: the split records of one gene's columns over the sorted union as the kernel wrote them ->
        list of (column, split as an int with taxon i = bit i), in record order"""
        keep = []
        a = _aln_struct(gene[0], gene[1], keep)
        nu = len(names_union)
        na = (C.c_char_p * nu)(*[s.encode() for s in names_union])
        nrec, w, out = C.c_longlong(), C.c_int(), C.c_void_p()
        self._check(self.L.pml_debug_column_splits(self.ptr, C.byref(a), nu, na, C.byref(nrec), C.byref(w), C.byref(out)))
        try:
            flat = np.frombuffer(C.string_at(out, 8 * nrec.value * (w.value + 1)), dtype=np.uint64).reshape(nrec.value, w.value + 1)
            return [(int(r[0]), sum(int(r[1 + x]) << (64 * x) for x in range(w.value))) for r in flat]
        finally:
            self.L.pml_free(out)

    def pairscore_sum_stats(self):
        """k_pairscore_sum launches on this context so far and (profile mode) their summed HIP-event time in ms"""
        n, ms = C.c_longlong(), C.c_double()
        self._check(self.L.pml_pairscore_sum_stats(self.ptr, C.byref(n), C.byref(ms)))
        return {"launches": n.value, "ms": ms.value}

    def debug_replicate_freqs(self, genes, sel=None):
        """Test hook for k_codehist: the code histogram of the device-gathered selection (None = all genes) and the empirical
        frequencies counted from it -> (counts int64[23], pi float64[20])."""
        keep = []
        n = len(genes)
        alns = (_lib.Alignment * n)(*[_aln_struct(g[0], g[1], keep) for g in genes])
        counts, pi = np.zeros(23, dtype=np.int64), np.zeros(20)
        arr = (C.c_int * len(sel))(*sel) if sel is not None else None
        rc = self.L.pml_debug_replicate_freqs(self.ptr, n, alns, len(sel) if sel is not None else 0, arr,
                                              counts.ctypes.data_as(C.POINTER(C.c_longlong)), _dp(pi))
        self._check(rc)
        return counts, pi

    def debug_gather(self, genes, sel=None):
        """Test hook: the replicate code matrix k_gather builds on the device for the gene selection,
        read back -> (names, codes uint8[ntax, npat], weights float64[npat])."""
        import numpy as np
        keep = []
        n = len(genes)
        alns = (_lib.Alignment * n)(*[_aln_struct(g[0], g[1], keep) for g in genes])
        nt, npat, mpad = C.c_int(), C.c_int(), C.c_int()
        codes, w, names = C.c_void_p(), C.c_void_p(), C.c_void_p()
        arr = (C.c_int * len(sel))(*sel) if sel is not None else None
        rc = self.L.pml_debug_gather(self.ptr, n, alns, len(sel) if sel is not None else 0, arr, C.byref(nt), C.byref(npat),
                                     C.byref(mpad), C.byref(codes), C.byref(w), C.byref(names))
        self._check(rc)
        cm = np.frombuffer(C.string_at(codes, nt.value * mpad.value), dtype=np.uint8).reshape(nt.value, mpad.value).copy()
        wv = np.frombuffer(C.string_at(w, 8 * mpad.value), dtype=np.float64).copy()
        nm = C.string_at(names).decode().splitlines()
        for p in (codes, w, names):
            self.L.pml_free(p)
        assert np.all(wv[npat.value:] == 0) and np.all(cm[:, npat.value:] == 22), "padding patterns must be weightless gaps"
        return nm, cm[:, :npat.value], wv[:npat.value]

    # ---- single-gene calls (what one Java thread issues); concurrent ones are coalesced inside the library ----
    def _single(self, fn, gene, newick, model, extra):
        keep = []
        a = _aln_struct(gene[0], gene[1], keep)
        res = _lib.Result()
        rc = fn(self.ptr, C.byref(a), newick.encode() if newick is not None else None, C.byref(model), *extra, C.byref(res))
        d = None
        if rc == 0:
            d = {"lnl": res.lnl, "alpha": res.alpha, "tree_length": res.tree_length, "npatterns": res.npatterns,
                 "nsites": res.nsites, "newick": C.string_at(res.newick).decode() if res.newick else None}
        self.L.pml_result_free(C.byref(res))
        self._check(rc)
        return d

    def score_one(self, gene, newick, alpha=1.0, ncat=4, pi_mode=PI_RAXML_3DP):
        return self._single(self.L.pml_score, gene, newick, _model(ncat, alpha, pi_mode), (0,))

    def optimize_one(self, gene, newick, alpha=1.0, ncat=4, pi_mode=PI_RAXML_3DP, optimize_alpha=True, epsilon=1e-4):
        o = _opts(optimize_alpha, False, 0, epsilon)
        return self._single(self.L.pml_optimize, gene, newick, _model(ncat, alpha, pi_mode), (C.byref(o),))

    def search_one(self, gene, start=None, alpha=1.0, ncat=4, pi_mode=PI_RAXML_3DP, optimize_alpha=True, nni=True,
                   spr_radius=0, epsilon=1e-3):
        o = _opts(optimize_alpha, nni, spr_radius, epsilon)
        return self._single(self.L.pml_search, gene, start, _model(ncat, alpha, pi_mode), (C.byref(o),))

    def coalescing_stats(self):
        b, r = C.c_longlong(), C.c_longlong()
        self._check(self.L.pml_coalescing_stats(self.ptr, C.byref(b), C.byref(r)))
        return {"batches": b.value, "requests": r.value}

    def register_matrix(self, name, exch190, pi20):
        """-> model code: `code` = this matrix with its own frequencies, `code + 1` = with each gene's empirical frequencies"""
        ex, pi = np.ascontiguousarray(exch190, dtype=np.float64), np.ascontiguousarray(pi20, dtype=np.float64)
        assert ex.shape == (190,) and pi.shape == (20,)
        code = C.c_int()
        self._check(self.L.pml_matrix_register(self.ptr, name.encode(), _dp(ex), _dp(pi), C.byref(code)))
        return code.value

    def model_eval(self, gene, newick, codes, optimize_alpha=True, epsilon=1e-4):
        """one tree optimised under each model code in ONE device batch -> (results as optimize_one gives them, index of the best)"""
        keep = []
        aln = _aln_struct(gene[0], gene[1], keep)
        n = len(codes)
        cs = (C.c_int * n)(*codes)
        o = _opts(optimize_alpha, False, 0, epsilon)
        res = (_lib.Result * n)()
        best = C.c_int(-1)
        rc = self.L.pml_model_eval(self.ptr, C.byref(aln), newick.encode(), n, cs, C.byref(o), res, C.byref(best))
        out = []
        if rc == 0:
            out = [{"lnl": r.lnl, "alpha": r.alpha, "tree_length": r.tree_length, "npatterns": r.npatterns, "nsites": r.nsites,
                    "newick": C.string_at(r.newick).decode() if r.newick else None} for r in res]
        for r in res:
            self.L.pml_result_free(C.byref(r))
        self._check(rc)
        return out, best.value

    def debug_model_build(self, exch, pi):
        """k_model on n matrices (n x 190, n x 20) -> list of dicts eval / U / Uinv / pi / UinvT, and the raw n x 1240 array"""
        ex, p = np.ascontiguousarray(exch, dtype=np.float64), np.ascontiguousarray(pi, dtype=np.float64)
        n = ex.shape[0]
        assert ex.shape == (n, 190) and p.shape == (n, 20)
        raw = np.zeros((n, MODELDEV_DOUBLES))
        self._check(self.L.pml_debug_model_build(self.ptr, n, _dp(ex), _dp(p), _dp(raw)))
        out = [{"eval": r[:20].copy(), "U": r[20:420].reshape(20, 20).copy(), "Uinv": r[420:820].reshape(20, 20).copy(),
                "pi": r[820:840].copy(), "UinvT": r[840:1240].reshape(20, 20).copy()} for r in raw]
        return out, raw

    # ---- tree selection tests (TreeComparison.runConsel: makermt | consel | catpv) ----
    @staticmethod
    def _test_opts(scales, reps, seed, keep):
        o = _lib.TreeTestOpts(0, None, int(reps), int(seed))
        if scales is not None:
            sc = np.ascontiguousarray(scales, dtype=np.float64)
            keep.append(sc)
            o.nscales, o.scales = len(sc), _dp(sc)
        return o

    def _test_result(self, res):
        T, K = res.ntrees, res.nscales

        def arr(p, n, dt):
            return np.ctypeslib.as_array(p, shape=(n,)).astype(dt, copy=True)
        out = {"ntrees": T, "nscales": K, "k1": res.k1, "nsites": res.nsites, "reps": res.reps,
               "scales": arr(res.scales, K, np.float64), "ndraws": arr(res.ndraws, K, np.int64),
               "au_nused": arr(res.au_nused, T, np.int64), "rank": arr(res.rank, T, np.int64),
               "bp_count": arr(res.bp_count, K * T, np.int64).reshape(K, T),
               "kh_count": arr(res.kh_count, T, np.int64), "sh_count": arr(res.sh_count, T, np.int64)}
        for f in ("lnl", "obs", "au", "np", "bp", "kh", "sh", "pp", "au_d", "au_c", "au_rss"):
            out[f] = arr(getattr(res, f), T, np.float64)
        return out

    def _weighted_result(self, w):
        T = w.ntrees

        def arr(p, n, dt):
            return np.ctypeslib.as_array(p, shape=(n,)).astype(dt, copy=True)
        return {"wkh": arr(w.wkh, T, np.float64), "wsh": arr(w.wsh, T, np.float64), "wkh_count": arr(w.wkh_count, T, np.int64),
                "wsh_count": arr(w.wsh_count, T, np.int64), "sigma": arr(w.sigma, T * T, np.float64).reshape(T, T),
                "wkh_other": arr(w.wkh_other, T, np.int64)}

    def rell_tests(self, site_lnl, scales=None, reps=10000, seed=0, weighted=False):
        """AU / KH / SH / BP of T trees from their per-site lnL (T x N, the rows of RAxML_perSiteLLs): multiscale RELL on the
        device.  scales None = 0.5 ... 1.4; reps per scale (PEPR's `makermt -b 10`: 100000).  -> dict of per-tree arrays
        (lnl, obs, au, np, bp, kh, sh, pp, au_d, au_c, au_rss, au_nused, rank) and the raw counts bp_count[K, T], kh_count, sh_count.
        weighted=True (pml_rell_tests_weighted): the same values plus wkh, wsh, wkh_count, wsh_count, sigma[T, T], wkh_other."""
        x = np.ascontiguousarray(site_lnl, dtype=np.float64)
        if x.ndim != 2:
            raise ValueError("site_lnl must be trees x sites")
        keep = []
        o = self._test_opts(scales, reps, seed, keep)
        res, w = _lib.TreeTestResult(), _lib.TreeTestWeighted()
        if weighted:
            rc = self.L.pml_rell_tests_weighted(self.ptr, x.shape[1], x.shape[0], _dp(x), C.byref(o), C.byref(res), C.byref(w))
        else:
            rc = self.L.pml_rell_tests(self.ptr, x.shape[1], x.shape[0], _dp(x), C.byref(o), C.byref(res))
        self._check(rc)
        out = self._test_result(res)
        self.L.pml_tree_test_result_free(C.byref(res))
        if weighted:
            out.update(self._weighted_result(w))
            self.L.pml_tree_test_weighted_free(C.byref(w))
        return out

    def tree_tests(self, gene, newicks, alpha=1.0, ncat=4, pi_mode=PI_RAXML_3DP, optimize=True, optimize_alpha=True, epsilon=1e-4,
                   scales=None, reps=10000, seed=0, weighted=False):
        """The whole runConsel chain for one alignment and T candidate trees in one call: every tree optimised (optimize=False:
        scored as given) in one device batch, the per-site lnL table built and resampled on the device.  -> the dict of
        rell_tests plus "site_lnl" (T x N, the very values that were resampled); weighted=True adds the keys rell_tests adds."""
        keep = []
        a = _aln_struct(gene[0], gene[1], keep)
        T = len(newicks)
        nw = (C.c_char_p * T)(*[s.encode() for s in newicks])
        m = _model(ncat, alpha, pi_mode)
        so = _opts(optimize_alpha, False, 0, epsilon)
        o = self._test_opts(scales, reps, seed, keep)
        res, w = _lib.TreeTestResult(), _lib.TreeTestWeighted()
        site = np.zeros((T, max(a.nsites, 1)))
        if weighted:
            rc = self.L.pml_tree_tests_weighted(self.ptr, C.byref(a), T, nw, C.byref(m), C.byref(so) if optimize else None, C.byref(o), C.byref(res),
                                                C.byref(w), _dp(site))
        else:
            rc = self.L.pml_tree_tests(self.ptr, C.byref(a), T, nw, C.byref(m), C.byref(so) if optimize else None, C.byref(o), C.byref(res), _dp(site))
        self._check(rc)
        out = self._test_result(res)
        self.L.pml_tree_test_result_free(C.byref(res))
        if weighted:
            out.update(self._weighted_result(w))
            self.L.pml_tree_test_weighted_free(C.byref(w))
        out["site_lnl"] = site[:, :a.nsites]
        return out

    def debug_rell(self, site_lnl, ndraws, reps, seed=0, path=0, want_y=True, weighted=False, inv_sigma=None):
        """Test door of k_rell: scale k draws ndraws[k] sites.  path 0 = auto, 1 = LDS, 2 = global memory.
        -> {"Y": [K, reps, T] replicate sums (None unless want_y), "bp": [K, T], "kh": [T], "sh": [T], "path": 1 | 2, "ms": kernel time}
        weighted=True (or an inv_sigma matrix [T, T]): the weighted arm through pml_debug_rell_weighted, with inv_sigma None
        computed by k_rell_pairsd; adds "wkh", "wsh" [T] and "inv_sigma" [T, T], the matrix that was used."""
        x = np.ascontiguousarray(site_lnl, dtype=np.float64)
        T, N = x.shape
        nd = np.ascontiguousarray(ndraws, dtype=np.int64)
        K = len(nd)
        lp = C.POINTER(C.c_longlong)
        y = np.zeros((K, reps, T)) if want_y else None
        bp, kh, sh = np.zeros((K, T), dtype=np.int64), np.zeros(T, dtype=np.int64), np.zeros(T, dtype=np.int64)
        used, ms = C.c_int(0), C.c_double(0)
        if not weighted and inv_sigma is None:
            rc = self.L.pml_debug_rell(self.ptr, N, T, _dp(x), K, nd.ctypes.data_as(lp), int(reps), int(seed), int(path), _dp(y) if want_y else None,
                                       bp.ctypes.data_as(lp), kh.ctypes.data_as(lp), sh.ctypes.data_as(lp), C.byref(used), C.byref(ms))
            self._check(rc)
            return {"Y": y, "bp": bp, "kh": kh, "sh": sh, "path": used.value, "ms": ms.value}
        isin = None if inv_sigma is None else np.ascontiguousarray(inv_sigma, dtype=np.float64)
        if isin is not None and isin.shape != (T, T):
            raise ValueError("inv_sigma must be trees x trees")
        isout, wkh, wsh = np.zeros((T, T)), np.zeros(T, dtype=np.int64), np.zeros(T, dtype=np.int64)
        rc = self.L.pml_debug_rell_weighted(self.ptr, N, T, _dp(x), K, nd.ctypes.data_as(lp), int(reps), int(seed), int(path),
                                            _dp(y) if want_y else None, bp.ctypes.data_as(lp), kh.ctypes.data_as(lp), sh.ctypes.data_as(lp),
                                            C.byref(used), C.byref(ms), _dp(isin) if isin is not None else None, _dp(isout),
                                            wkh.ctypes.data_as(lp), wsh.ctypes.data_as(lp))
        self._check(rc)
        return {"Y": y, "bp": bp, "kh": kh, "sh": sh, "path": used.value, "ms": ms.value, "wkh": wkh, "wsh": wsh, "inv_sigma": isout}

    def newton_fallbacks(self):
        """how often k_newton's bounded exchange wait gave up on this context and work was re-issued through the no-exchange form"""
        a, b, c = C.c_longlong(), C.c_longlong(), C.c_longlong()
        self._check(self.L.pml_newton_fallbacks(self.ptr, C.byref(a), C.byref(b), C.byref(c)))
        return {"giveups": a.value, "reissued": b.value, "seq_launches": c.value}

    def kernel_stats(self, reset=False):
        out = {}
        for name, k in KERNELS.items():
            n, ms, by = C.c_longlong(), C.c_double(), C.c_double()
            self._check(self.L.pml_kernel_stats(self.ptr, k, C.byref(n), C.byref(ms), C.byref(by)))
            fl = C.c_double()
            self._check(self.L.pml_kernel_flops(self.ptr, k, C.byref(fl)))
            out[name] = {"launches": n.value, "ms": ms.value, "algo_bytes": by.value, "algo_flops": fl.value}
        if reset:
            self.L.pml_kernel_stats_reset(self.ptr)
        return out


class Batch:
    """Genes encoded and resident in HBM; repeated evaluation without host transfers."""

    def __init__(self, ctx, genes, newicks=None, alpha=1.0, ncat=4, pi_mode=PI_RAXML_3DP):
        self.ctx, self.L = ctx, ctx.L
        keep = []
        n = len(genes)
        alns = (_lib.Alignment * n)(*[_aln_struct(g[0], g[1], keep) for g in genes])
        nw = None
        if newicks is not None:
            nw = (C.c_char_p * n)(*[(s.encode() if s is not None else None) for s in newicks])
        m = _model(ncat, alpha, pi_mode)
        self.ptr = C.c_void_p()
        ctx._check(self.L.pml_batch_create(ctx.ptr, n, alns, nw, C.byref(m), C.byref(self.ptr)))
        self.n = n

    def close(self):
        if self.ptr:
            self.L.pml_batch_destroy(self.ptr)
            self.ptr = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def npatterns(self):
        return [self.L.pml_batch_npatterns(self.ptr, g) for g in range(self.n)]

    def score(self, stored=False):
        """full post-order pass + root evaluation of every gene; stored=True writes every CLV (the traversal a search runs)"""
        out = np.zeros(self.n)
        fn = self.L.pml_batch_score_stored if stored else self.L.pml_batch_score
        self.ctx._check(fn(self.ptr, out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def site_lnl(self, g, nsites):
        out = np.zeros(max(nsites, 1))
        self.ctx._check(self.L.pml_batch_site_lnl(self.ptr, g, out.ctypes.data_as(C.POINTER(C.c_double))))
        return out[:nsites]

    def set_alpha(self, alpha, g=-1):
        self.ctx._check(self.L.pml_batch_set_alpha(self.ptr, g, alpha))

    def set_matrix(self, exch190, pi20=None, g=-1):
        """the rate matrix of gene g (-1: all genes); pi20 None keeps the frequencies.  Any batch becomes a per-gene-model batch."""
        ex = np.ascontiguousarray(exch190, dtype=np.float64)
        pi = None if pi20 is None else np.ascontiguousarray(pi20, dtype=np.float64)
        assert ex.shape == (190,) and (pi is None or pi.shape == (20,))
        self.ctx._check(self.L.pml_batch_set_matrix(self.ptr, g, _dp(ex), None if pi is None else _dp(pi)))

    def get_matrix(self, g):
        """(exchangeabilities, frequencies) gene g is scored with: estimates after a GTR optimisation, counted frequencies of F variants"""
        ex, pi = np.zeros(190), np.zeros(20)
        self.ctx._check(self.L.pml_batch_get_matrix(self.ptr, g, _dp(ex), _dp(pi)))
        return ex, pi

    def root_derivs(self):
        a, b, c = np.zeros(self.n), np.zeros(self.n), np.zeros(self.n)
        dp = C.POINTER(C.c_double)
        self.ctx._check(self.L.pml_batch_root_derivs(self.ptr, a.ctypes.data_as(dp), b.ctypes.data_as(dp), c.ctypes.data_as(dp)))
        return a, b, c

    def optimize(self, optimize_alpha=True, epsilon=1e-4):
        o = _opts(optimize_alpha, False, 0, epsilon)
        lnl, al = np.zeros(self.n), np.zeros(self.n)
        dp = C.POINTER(C.c_double)
        self.ctx._check(self.L.pml_batch_optimize(self.ptr, C.byref(o), lnl.ctypes.data_as(dp), al.ctypes.data_as(dp)))
        return lnl, al

    def search(self, optimize_alpha=True, nni=True, spr_radius=0, epsilon=1e-3, constraints=None):
        o = _opts(optimize_alpha, nni, spr_radius, epsilon, constraints=constraints)
        lnl, al = np.zeros(self.n), np.zeros(self.n)
        dp = C.POINTER(C.c_double)
        self.ctx._check(self.L.pml_batch_search(self.ptr, C.byref(o), lnl.ctypes.data_as(dp), al.ctypes.data_as(dp)))
        return lnl, al

    def newick(self, g, digits=10):
        p = C.c_void_p()
        self.ctx._check(self.L.pml_batch_newick(self.ptr, g, digits, C.byref(p)))
        s = C.string_at(p).decode()
        self.L.pml_free(p)
        return s


def catpv_table(result, weighted=None):
    """Host-only (pml_catpv_table): the lines of the `catpv -v`-shaped table -- a header and one line per tree in rank order,
    columns rank item obs au np | bp pp kh sh wkh wsh | -- from a result dict of rell_tests / tree_tests.  weighted: None = the
    result's own wkh / wsh if it has them (else the two columns print "-"), or a dict that holds them."""
    L = _lib.load()
    T = int(result["ntrees"])
    keep = {f: np.ascontiguousarray(result[f], dtype=np.float64) for f in ("obs", "au", "np", "bp", "pp", "kh", "sh")}
    rank = np.ascontiguousarray(result["rank"], dtype=np.int32)
    res = _lib.TreeTestResult()
    res.ntrees = T
    res.rank = rank.ctypes.data_as(C.POINTER(C.c_int))
    for f, a in keep.items():
        if a.shape != (T,):
            raise ValueError(f + " must hold one value per tree")
        setattr(res, f, _dp(a))
    if rank.shape != (T,):
        raise ValueError("rank must hold one value per tree")
    wsrc = weighted if weighted is not None else (result if "wkh" in result and "wsh" in result else None)
    w, wp = _lib.TreeTestWeighted(), None
    if wsrc is not None:
        wk, ws = (np.ascontiguousarray(wsrc[f], dtype=np.float64) for f in ("wkh", "wsh"))
        if wk.shape != (T,) or ws.shape != (T,):
            raise ValueError("wkh / wsh must hold one value per tree")
        w.ntrees, w.wkh, w.wsh = T, _dp(wk), _dp(ws)
        wp = C.byref(w)
    out = C.c_void_p()
    rc = L.pml_catpv_table(C.byref(res), wp, C.byref(out))
    if rc != 0:
        raise PmlError(rc, "pml_catpv_table")
    txt = C.string_at(out).decode()
    L.pml_free(out)
    return txt.split("\n")


def au_fit(r, count, B):
    """Shimodaira's AU p-value from the bootstrap counts of one tree at the scales r (= n_k / N); host only.
    -> {"au", "d", "c", "rss", "nused"}"""
    L = _lib.load()
    rr = np.ascontiguousarray(r, dtype=np.float64)
    cc = np.ascontiguousarray(count, dtype=np.int64)
    if rr.shape != cc.shape or rr.ndim != 1:
        raise ValueError("r and count must be vectors of one length")
    au, d, c, rss, nused = C.c_double(), C.c_double(), C.c_double(), C.c_double(), C.c_int()
    rc = L.pml_au_fit(len(rr), _dp(rr), cc.ctypes.data_as(C.POINTER(C.c_longlong)), int(B), C.byref(au), C.byref(d), C.byref(c),
                      C.byref(rss), C.byref(nused))
    if rc:
        raise PmlError(rc)
    return {"au": au.value, "d": d.value, "c": c.value, "rss": rss.value, "nused": nused.value}


def format_double(x):
    """a double as text that reads back to the same bits: the shortest of %.15g, %.16g, %.17g that does (nj.hpp nj_number's
    rule, the spelling of every number this project prints: `0` for Java's `0.0`); NaN and infinities as Java spells them"""
    x = float(x)
    if x != x:
        return "NaN"
    if x in (float("inf"), float("-inf")):
        return "Infinity" if x > 0 else "-Infinity"
    for p in (15, 16, 17):
        s = "%.*g" % (p, x)
        if float(s) == x:
            return s
    return s


def rf_distance(newick_a, newick_b):
    L = _lib.load()
    rf = C.c_int()
    rc = L.pml_rf_distance(newick_a.encode(), newick_b.encode(), C.byref(rf))
    if rc:
        raise PmlError(rc, L.pml_last_error(None).decode())
    return rf.value


def fpenv_seen():
    """MXCSR control states callers entered the library with (diagnostic; the library computes under the default state)."""
    L = _lib.load()
    if not hasattr(L, "pml_debug_fpenv"):          # an older build loaded through PEPRML_LIB (A/B runs)
        return []
    v = (C.c_uint * 16)()
    n = L.pml_debug_fpenv(v, 16)
    return [int(x) for x in v[:min(n, 16)]]


def refine_next(supported_newick, cutoff=100, done=()):
    """Next clade to refine (PhylogeneticTreeRefiner.getNextIndexToRefine :298-359): (sorted leaf list or None,
    floor(mean descendant support) per node in order of appearance)."""
    L = _lib.load()
    n = len(done)
    arr = (C.c_char_p * max(n, 1))(*[",".join(sorted(d)).encode() for d in done]) if n else None
    p, nn, mp = C.c_void_p(), C.c_int(), C.c_void_p()
    rc = L.pml_refine_next(supported_newick.encode(), cutoff, n, arr, C.byref(p), C.byref(nn), C.byref(mp))
    if rc:
        raise PmlError(rc, L.pml_last_error(None).decode())
    ingroup = C.string_at(p).decode().split(",") if p else None
    means = list(C.cast(mp, C.POINTER(C.c_int))[:nn.value]) if mp else []
    if p:
        L.pml_free(p)
    if mp:
        L.pml_free(mp)
    return ingroup, means


def support_tree(main_newick, support_newicks, digits=6):
    """Main tree decorated with integer bipartition counts (TreeSupportDecorator.addSupportValues)."""
    L = _lib.load()
    n = len(support_newicks)
    arr = (C.c_char_p * max(n, 1))(*[s.encode() for s in support_newicks]) if n else None
    p = C.c_void_p()
    rc = L.pml_support_tree(main_newick.encode(), n, arr, digits, C.byref(p))
    if rc:
        raise PmlError(rc, L.pml_last_error(None).decode())
    s = C.string_at(p).decode()
    L.pml_free(p)
    return s


def support_tree_rule(main_newick, support_newicks, rule=SUPPORT_DECORATOR, digits=6):
    """support_tree() under a SUPPORT_* rule; the support trees may cover other taxon sets than the main tree's."""
    L = _lib.load()
    n = len(support_newicks)
    arr = (C.c_char_p * max(n, 1))(*[s.encode() for s in support_newicks]) if n else None
    p = C.c_void_p()
    rc = L.pml_support_tree_rule(main_newick.encode(), n, arr, int(rule), digits, C.byref(p))
    if rc:
        raise PmlError(rc, L.pml_last_error(None).decode())
    s = C.string_at(p).decode()
    L.pml_free(p)
    return s


def jackknife_draw(ngenes, reps, subset_size=0, seed=0):
    """The gene subsets pml_jackknife draws (host only): list of `reps` ascending index lists."""
    L = _lib.load()
    k = subset_size if subset_size > 0 else max(1, ngenes // 2)
    k = max(1, min(k, ngenes))
    out = (C.c_int * (reps * k))()
    rc = L.pml_jackknife_draw(ngenes, reps, subset_size, seed, out)
    if rc < 0:
        raise PmlError(rc)
    assert rc == k
    return [list(out[r * k:(r + 1) * k]) for r in range(reps)]


def jackknife_parsimony_seeds(seed, reps):
    """Host only: the stepwise-addition seeds of pml_jackknife3's parsimony trees -> (full tree's seed, [replicate r's seed]):
    (unsigned)seed and (unsigned)(seed + 1 + r), r = the replicate's index in jackknife_draw's list; 0 ("input order" to
    pml_parsimony) is replaced by 0x9E3779B9."""
    def u32(v):
        return (v & 0xFFFFFFFF) or 0x9E3779B9
    return u32(seed), [u32(seed + 1 + r) for r in range(reps)]


def congruence_select(mean_costs, trim_percent=0.1):
    """Host only: filterForCongruence's selection on the genes' mean costs -> {"keep", "idx", "max_cost"}; a trim_percent of 1.0
    or more is divided by 100; gene g is kept iff g <= idx and its mean cost <= max_cost (the Java's rule, position against rank).
    trim_percent <= 0, NaN or an index outside the genes: PmlError(EINVAL)."""
    L = _lib.load()
    n = len(mean_costs)
    m = (C.c_longlong * n)(*[int(x) for x in mean_costs])
    keep, idx, mx = (C.c_int * n)(), C.c_int(), C.c_longlong()
    rc = L.pml_congruence_select(n, m, float(trim_percent), keep, C.byref(idx), C.byref(mx))
    if rc:
        raise PmlError(rc, "trim_percent %r with %d genes" % (trim_percent, n))
    return {"keep": [bool(k) for k in keep], "idx": idx.value, "max_cost": mx.value}


def trim_column_flags_host(gene):
    """pml_trim_column_flags_host: Context.debug_column_flags' bytes from the same decision function on the host (no device)"""
    keep = []
    a = _raw_aln_struct(gene[0], gene[1], keep)
    out = np.zeros(max(a.nsites, 1), dtype=np.uint8)
    rc = _lib.load().pml_trim_column_flags_host(C.byref(a), out.ctypes.data_as(C.POINTER(C.c_ubyte)))
    if rc:
        raise PmlError(rc)
    return out[:a.nsites]


def gblocks_defaults(ntax):
    """pml_gblocks_defaults: PEPR's Gblocks parameters for a gene of ntax rows -> {"b1", "b2", "b3", "b4", "b0", "gaps"}"""
    p = _lib.GblocksParams()
    rc = _lib.load().pml_gblocks_defaults(int(ntax), C.byref(p))
    if rc:
        raise PmlError(rc, "ntax %r" % (ntax,))
    return {k: getattr(p, k) for k in ("b1", "b2", "b3", "b4", "b0", "gaps")}


def gblocks_flags_host(gene, params=None):
    """pml_gblocks_flags_host: Context.debug_gblocks_flags' bytes from the same functions on the host (no device)"""
    keep = []
    a = _raw_aln_struct(gene[0], gene[1], keep)
    out = np.zeros(max(a.nsites, 1), dtype=np.uint8)
    rc = _lib.load().pml_gblocks_flags_host(C.byref(a), _gblocks_params(params), out.ctypes.data_as(C.POINTER(C.c_ubyte)))
    if rc:
        raise PmlError(rc)
    return out[:a.nsites]


def gblocks_chunk():
    """the columns k_gbselect scans at a time"""
    return _lib.load().pml_gblocks_chunk()


MASH_INVALID = 0xFFFFFFFFFFFFFFFF     # what k_mash_hash writes where no valid window starts


def _ulp(a):
    return a.ctypes.data_as(C.POINTER(C.c_ulonglong))


def _genome_array(genomes, keep):
    """genomes (each a list of records, bytes or str) as the pml_genome array the C ABI takes; a str is its latin-1 bytes"""
    n = len(genomes)
    arr = (_lib.Genome * max(n, 1))()
    for g, recs in enumerate(genomes):
        recs = [r.encode("latin-1") if isinstance(r, str) else bytes(r) for r in recs]
        ra = (C.c_char_p * max(len(recs), 1))(*recs)
        la = (C.c_longlong * max(len(recs), 1))(*[len(r) for r in recs])
        keep.extend([recs, ra, la])
        arr[g] = _lib.Genome(len(recs), ra, la)
    keep.append(arr)
    return arr


def _sketch_rows(sketches, s):
    n = len(sketches)
    rows, lens = np.zeros((max(n, 1), s), dtype=np.uint64), np.zeros(max(n, 1), dtype=np.int32)
    for g, sk in enumerate(sketches):
        sk = np.asarray(sk, dtype=np.uint64)
        if sk.size > s:
            raise PmlError(EINVAL, "sketch %d has %d values, more than s = %d" % (g, sk.size, s))
        rows[g, :sk.size] = sk
        lens[g] = sk.size
    return rows, lens


def mash_tile():
    """the window starts k_mash_hash stages at a time"""
    return _lib.load().pml_mash_tile()


def mash_chunk():
    """the sketch values k_mash_pairs takes at a time"""
    return _lib.load().pml_mash_chunk()


def mash_murmur3(data, seed=0):
    """Host only: MurmurHash3_x64_128 of bytes -> (h1, h2)"""
    out = (C.c_ulonglong * 2)()
    rc = _lib.load().pml_mash_murmur3(data, len(data), int(seed), out)
    if rc:
        raise PmlError(rc)
    return out[0], out[1]


def mash_hashes_host(genome, k=21):
    """Host only: Context.debug_mash_hashes' values from the rule over bytes"""
    keep = []
    n = sum(len(r) for r in genome)
    out = np.zeros(max(n, 1), dtype=np.uint64)
    rc = _lib.load().pml_mash_hashes_host(_genome_array([genome], keep), int(k), _ulp(out))
    if rc:
        raise PmlError(rc, "k %r" % (k,))
    return out[:n]


def mash_sketch_host(genome, k=21, s=100000):
    """Host only: one genome's sketch"""
    keep = []
    out, n = np.zeros(max(int(s), 1), dtype=np.uint64), C.c_int()
    rc = _lib.load().pml_mash_sketch_host(_genome_array([genome], keep), int(k), int(s), _ulp(out), C.byref(n))
    if rc:
        raise PmlError(rc, "k %r, s %r" % (k, s))
    return out[:n.value].copy()


def _arc_arrays(arcs):
    arcs = list(arcs)
    a = np.ascontiguousarray([t[0] for t in arcs], dtype=np.int32)
    b = np.ascontiguousarray([t[1] for t in arcs], dtype=np.int32)
    w = np.ascontiguousarray([t[2] for t in arcs], dtype=np.float64)
    return a, b, w


def _clusters_of(cluster_of, nclusters):
    out = [[] for _ in range(nclusters)]
    for i, k in enumerate(cluster_of):
        out[int(k)].append(i)
    return out


def mcl_cluster_host(n, arcs, inflation=0.0, prune_inverse=0.0, chaos_eps=0.0, max_iter=0):
    """Host only: Context.mcl_cluster's rule in plain C++ loops (the CPU tests' subject and the timing baseline)"""
    a, b, w = _arc_arrays(arcs)
    out, nc, it = np.zeros(max(n, 1), dtype=np.int32), C.c_int(), C.c_int()
    o = _lib.MclOpts(float(inflation), float(prune_inverse), float(chaos_eps), int(max_iter), 0)
    ip = C.POINTER(C.c_int)
    rc = _lib.load().pml_mcl_cluster_host(int(n), a.size, a.ctypes.data_as(ip), b.ctypes.data_as(ip), _dp(w), C.byref(o), out.ctypes.data_as(ip), C.byref(nc), C.byref(it))
    if rc:
        raise PmlError(rc, "mcl_cluster_host")
    return {"clusters": _clusters_of(out[:n], nc.value), "cluster_of": out[:n].copy(), "iterations": it.value}


def _host_text(fn, *args):
    p = C.c_void_p()
    rc = fn(*args, C.byref(p))
    if rc:
        raise PmlError(rc, "the hit table")
    try:
        return C.string_at(p).decode()
    finally:
        _lib.load().pml_free(p)


def hits_filter_host(table):
    """Host only: filterHitPairFile (PhyloPipeline.java:989-1024) on a table's text"""
    t = table.encode() if isinstance(table, str) else bytes(table)
    return _host_text(_lib.load().pml_hits_filter_host, t, len(t))


def hits_bidirectional_host(table, score_field=11):
    """Host only: filterForBidirectional (PhyloPipeline.java:911-987) on a table's text"""
    t = table.encode() if isinstance(table, str) else bytes(table)
    return _host_text(_lib.load().pml_hits_bidirectional_host, t, len(t), int(score_field))


def homolog_select_host(clusters, taxon_of_node, min_taxa, max_taxa, rep_only, target_ntax, target_min_gene):
    """Host only: the set selection of createInputSequenceSetProvider on clusters of node indices -> kept cluster indices"""
    off = np.zeros(len(clusters) + 1, dtype=np.int64)
    for k, c in enumerate(clusters):
        off[k + 1] = off[k] + len(c)
    members = np.ascontiguousarray([i for c in clusters for i in c] or [0], dtype=np.int32)
    tax = np.ascontiguousarray(list(taxon_of_node) or [0], dtype=np.int32)
    kept, nk = np.zeros(max(len(clusters), 1), dtype=np.int32), C.c_int()
    ip = C.POINTER(C.c_int)
    rc = _lib.load().pml_homolog_select_host(len(clusters), off.ctypes.data_as(C.POINTER(C.c_longlong)), members.ctypes.data_as(ip), tax.ctypes.data_as(ip),
                                             int(min_taxa), int(max_taxa), int(bool(rep_only)), int(target_ntax), int(target_min_gene), kept.ctypes.data_as(ip), C.byref(nk))
    if rc:
        raise PmlError(rc, "homolog_select_host")
    return [int(k) for k in kept[:nk.value]]


def mcl_class_limits():
    """(the packed class's largest component, the LDS class's, the expansion tile)"""
    out = (C.c_int * 4)()
    _lib.load().pml_mcl_class_limits(out)
    return out[0], out[1], out[2]


def _sw_bytes(x):
    return x.encode("latin-1") if isinstance(x, str) else bytes(x)


def _sw_set(genomes, keep):
    off, labels, residues = [0], [], []
    for g in genomes:
        for title, res in g:
            labels.append(_sw_bytes(title))
            residues.append(_sw_bytes(res))
        off.append(len(labels))
    oa = (C.c_int * len(off))(*off)
    la = (C.c_char_p * max(len(labels), 1))(*labels)
    ra = (C.c_char_p * max(len(residues), 1))(*residues)
    keep += [oa, la, ra]
    return _lib.ProteomeSet(len(genomes), oa, la, ra)


def _sw_opts(opts, keep):
    bad = set(opts) - {"gap_open", "gap_extend", "lambda_", "K", "evalue", "hits_per_query", "traceback", "table"}
    if bad:
        raise TypeError("unknown option(s) " + ", ".join(sorted(bad)))
    o = _lib.SwOpts(int(opts.get("gap_open", 0)), int(opts.get("gap_extend", 0)), float(opts.get("lambda_", 0.0)), float(opts.get("K", 0.0)),
                    float(opts.get("evalue", 0.0)), int(opts.get("hits_per_query", 0)), int(bool(opts.get("traceback", False))), None)
    if opts.get("table") is not None:
        t = np.ascontiguousarray(opts["table"], dtype=np.int32).reshape(576)
        keep.append(t)
        o.table576 = t.ctypes.data_as(C.POINTER(C.c_int))
    return o


def _sw_result(r):
    try:
        n = r.nhits
        return {"table": C.string_at(r.table, r.table_bytes), "cells": r.cells,
                "query": [r.query[i] for i in range(n)], "subject": [r.subject[i] for i in range(n)],
                "target_genome": [r.target_genome[i] for i in range(n)], "score": [r.score[i] for i in range(n)],
                "bits": [r.bits[i] for i in range(n)], "evalue": [r.evalue[i] for i in range(n)]}
    finally:
        _lib.load().pml_sw_result_free(C.byref(r))


def sw_search_host(genomes, **opts):
    """Host only: Context.sw_search's rule in plain C++ loops (the CPU tests' subject and the timing baseline).  Options:
    gap_open, gap_extend, lambda_, K, evalue (0 = 11, 1, 0.267, 0.041, 0.1), hits_per_query (0 / 1), traceback, table (576 ints).
    -> {"table" (bytes, the twelve-field lines), "query", "subject" (global protein indices), "target_genome", "score", "bits",
    "evalue" per hit, "cells"}"""
    keep = []
    st, o, r = _sw_set(genomes, keep), _sw_opts(opts, keep), _lib.SwResult()
    rc = _lib.load().pml_sw_search_host(C.byref(st), C.byref(o), C.byref(r))
    if rc:
        raise PmlError(rc, "sw_search_host")
    return _sw_result(r)


def _msa_sets(sets, keep):
    arr = (_lib.MsaSet * max(len(sets), 1))()
    for i, st in enumerate(sets):
        ra = (C.c_char_p * max(len(st), 1))(*[_sw_bytes(x) for x in st])
        keep.append(ra)
        arr[i] = _lib.MsaSet(len(st), ra)
    keep.append(arr)
    return arr


def _msa_opts(opts, keep):
    bad = set(opts) - {"gap_open", "gap_extend", "table"}
    if bad:
        raise TypeError("unknown option(s) " + ", ".join(sorted(bad)))
    o = _lib.MsaOpts(int(opts.get("gap_open", 0)), int(opts.get("gap_extend", 0)), None)
    if opts.get("table") is not None:
        t = np.ascontiguousarray(opts["table"], dtype=np.int32).reshape(576)
        keep.append(t)
        o.table576 = t.ctypes.data_as(C.POINTER(C.c_int))
    return o


def _msa_result(r):
    try:
        rows = [C.string_at(r.rows + i * (r.ncols + 1), r.ncols).decode("latin-1") for i in range(r.nrows)]
        out = {"rows": rows, "merges": [(r.merge_x[m], r.merge_y[m], r.merge_level[m], r.merge_score[m]) for m in range(r.nmerges)]}
        if r.path:
            out["path"] = [r.path[c] for c in range(r.ncols)]
        return out
    finally:
        _lib.load().pml_msa_result_free(C.byref(r))


def msa_align_host(sets, **opts):
    """Host only: Context.msa_align's rule in plain C++ loops (the CPU tests' subject and the timing baseline)"""
    keep = []
    sa, o = _msa_sets(sets, keep), _msa_opts(opts, keep)
    res = (_lib.MsaResult * max(len(sets), 1))()
    err = C.create_string_buffer(512)
    rc = _lib.load().pml_msa_align_host(len(sets), sa, C.byref(o), res, err, 512)
    if rc:
        raise PmlError(rc, err.value.decode("latin-1"))
    return [_msa_result(res[i]) for i in range(len(sets))]


def msa_profile_align_host(a, b, **opts):
    """Host only: Context.msa_profile_align's rule in plain C++ loops"""
    keep = []
    sa, sb, o, r, sc = _msa_sets([a], keep), _msa_sets([b], keep), _msa_opts(opts, keep), _lib.MsaResult(), C.c_longlong()
    err = C.create_string_buffer(512)
    rc = _lib.load().pml_msa_profile_align_host(sa, sb, C.byref(o), C.byref(sc), C.byref(r), err, 512)
    if rc:
        raise PmlError(rc, err.value.decode("latin-1"))
    out = _msa_result(r)
    out["score"] = sc.value
    return out


def msa_guide_tree_host(scores):
    """Host only: the merges [(x, y, level)] of a set from its n x n pair scores (the entries above the diagonal are read)"""
    s = np.ascontiguousarray(scores, dtype=np.int64)
    n = s.shape[0]
    assert s.shape == (n, n)
    x, y, lv = (C.c_int * max(n - 1, 1))(), (C.c_int * max(n - 1, 1))(), (C.c_int * max(n - 1, 1))()
    rc = _lib.load().pml_msa_guide_tree_host(n, s.ctypes.data_as(C.POINTER(C.c_longlong)), x, y, lv)
    if rc:
        raise PmlError(rc, "msa_guide_tree_host")
    return [(x[m], y[m], lv[m]) for m in range(n - 1)]


def msa_limits():
    """{"lanes": group widths per class, "rows": the columns of X of one pass per class, "strip": T, "threads": a workgroup}"""
    out = (C.c_int * 8)()
    _lib.load().pml_msa_limits(out)
    return {"lanes": [out[0], out[2], out[4]], "rows": [out[1], out[3], out[5]], "strip": out[6], "threads": out[7]}


def sw_class_limits():
    """{"lanes": group widths per class, "rows": the longest query of one pass per class, "strip": T, "chunk": stream bytes}"""
    out = (C.c_int * 8)()
    _lib.load().pml_sw_class_limits(out)
    return {"lanes": [out[0], out[2], out[4]], "rows": [out[1], out[3], out[5]], "strip": out[6], "chunk": out[7]}


def mash_pair_host(a, b, s):
    """Host only: (common, denom) of two sketches by the sequential loop that defines them"""
    a, b = np.ascontiguousarray(a, dtype=np.uint64), np.ascontiguousarray(b, dtype=np.uint64)
    c, d = C.c_int(), C.c_int()
    rc = _lib.load().pml_mash_pair_host(_ulp(a), a.size, _ulp(b), b.size, int(s), C.byref(c), C.byref(d))
    if rc:
        raise PmlError(rc, "s %r" % (s,))
    return c.value, d.value


def mash_distance_of(common, denom, k, digits=None):
    """Host only: the distance of a pair's two integers; digits = 6 as NeighborMasher reads it from mash's text"""
    return _lib.load().pml_mash_distance_of(int(common), int(denom), int(k), int(digits or 0))


def _pool_table(d):
    d = np.ascontiguousarray(np.asarray(d, dtype=np.float64))
    if d.ndim != 2 or d.shape[1] < 1:
        raise PmlError(EINVAL, "the distance table must be pool x ingroup")
    return d


def mash_candidate_distances(d):
    """Host only: getMaxDistanceForEachOutgroupToIngroupSketch on a pool x ingroup table"""
    d = _pool_table(d)
    out = np.zeros(max(d.shape[0], 1))
    rc = _lib.load().pml_mash_candidate_distances(d.shape[1], d.shape[0], _dp(d), _dp(out))
    if rc:
        raise PmlError(rc)
    return out[:d.shape[0]]


def mash_expand_ingroup(d, target, pool_is_ingroup=None):
    """Host only: expandIngroup on a pool x ingroup table -> the pool indices added, in order"""
    d = _pool_table(d)
    n = d.shape[0]
    flags = None if pool_is_ingroup is None else (C.c_ubyte * max(n, 1))(*[int(bool(x)) for x in pool_is_ingroup])
    added, na = (C.c_int * max(n, 1))(), C.c_int()
    rc = _lib.load().pml_mash_expand_ingroup(d.shape[1], n, _dp(d), flags, int(target), added, C.byref(na))
    if rc:
        raise PmlError(rc)
    return [added[i] for i in range(na.value)]


def mash_pair_stats(distances):
    """Host only: StatisticsUtilities' mean, standard deviation and maximum as getIngroupPairDistances' caller uses them"""
    d = np.ascontiguousarray(np.asarray(distances, dtype=np.float64).reshape(-1))
    out = (C.c_double * 3)()
    rc = _lib.load().pml_mash_pair_stats(d.size, _dp(d) if d.size else None, out)
    if rc:
        raise PmlError(rc)
    return out[0], out[1], out[2]


def mash_select_outgroup(cand, max_ingroup, sd, count):
    """Host only: selectOutgroupCandidates -> the selected candidates' indices, in order"""
    c = np.ascontiguousarray(np.asarray(cand, dtype=np.float64).reshape(-1))
    sel, ns = (C.c_int * max(c.size, 1))(), C.c_int()
    rc = _lib.load().pml_mash_select_outgroup(c.size, _dp(c) if c.size else None, float(max_ingroup), float(sd), int(count), sel, C.byref(ns))
    if rc:
        raise PmlError(rc)
    return [sel[i] for i in range(ns.value)]


def _gene_steps_struct(result):
    """a gene_steps dict as the C struct the threshold calls read (the arrays stay the dict's; names are not needed)"""
    G = len(result["col_start"]) - 1
    keep = [np.ascontiguousarray(result[k], dtype=t) for k, t in (("col_start", np.int64), ("steps", np.int32), ("min_steps", np.int32),
                                                                   ("gene_steps", np.int64), ("gene_beyond", np.int64), ("gene_ratio", np.float32))]
    for a in (1, 2):
        if keep[a].size == 0:
            keep[a] = np.zeros(1, dtype=np.int32)
    ip, lp = C.POINTER(C.c_int), C.POINTER(C.c_longlong)
    res = _lib.GeneStepsResult(G, len(result.get("names", ())), None, int(keep[0][-1]) if G >= 0 and keep[0].size else 0, keep[0].ctypes.data_as(lp),
                               keep[1].ctypes.data_as(ip), keep[2].ctypes.data_as(ip), keep[3].ctypes.data_as(lp), keep[4].ctypes.data_as(lp),
                               keep[5].ctypes.data_as(C.POINTER(C.c_float)))
    return res, keep


def _step_opts(statistic, replace, multiple, reps, alpha, seed, mask, ngenes, keep):
    m = None
    if mask is not None:
        if len(mask) != ngenes:
            raise ValueError("mask needs one entry per gene")
        m = (C.c_ubyte * max(ngenes, 1))(*[1 if x else 0 for x in mask])
        keep.append(m)
    return _lib.StepThresholdOpts(int(statistic), int(bool(replace)), int(multiple), int(reps), float(alpha), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                  C.cast(m, C.POINTER(C.c_ubyte)) if m is not None else None)


def step_draws_host(col_start, gene, rep, statistic=STEPS_BEYOND_MIN, replace=True, multiple=3, reps=1000, alpha=0.05, seed=0, mask=None):
    """pml_step_draws_host: the concatenation columns replicate `rep` of `gene` draws, in draw order, from the draw functions the
    kernel runs (no device) -> int64 array of the gene's length"""
    cs = np.ascontiguousarray(col_start, dtype=np.int64)
    G = len(cs) - 1
    keep = []
    o = _step_opts(statistic, replace, multiple, reps, alpha, seed, mask, G, keep)
    lp = C.POINTER(C.c_longlong)
    n = int(cs[gene + 1] - cs[gene]) if 0 <= gene < G else 0
    out = np.zeros(max(n, 1), dtype=np.int64)
    rc = _lib.load().pml_step_draws_host(C.byref(o), G, cs.ctypes.data_as(lp), int(gene), int(rep), out.ctypes.data_as(lp))
    if rc:
        raise PmlError(rc)
    return out[:n]


def boot_draws_host(seed, rep, ncols):
    """pml_boot_draws_host: the ncols columns replicate `rep` of a bootstrap2 call with `seed` draws, in draw order, from the
    functions the kernel runs (no device) -> uint32 array"""
    out = np.zeros(max(int(ncols), 1) if int(ncols) < (1 << 31) else 1, dtype=np.uint32)
    rc = _lib.load().pml_boot_draws_host(int(seed) & 0xFFFFFFFFFFFFFFFF, int(rep), int(ncols), out.ctypes.data_as(C.POINTER(C.c_uint)))
    if rc:
        raise PmlError(rc, "rep %r, ncols %r" % (rep, ncols))
    return out[:ncols]


def boot_tile():
    """the patterns k_boot_index compacts per step of its scan"""
    return _lib.load().pml_boot_tile()


def congruence_ktile():
    """the kept splits k_splitcost holds in LDS at a time"""
    return _lib.load().pml_congruence_ktile()


def concatenate(genes, sel=None):
    """Sorted-taxon-union concatenation with '?' padding (MSAConcatenator.java:78-189) -> (names, rows)."""
    L = _lib.load()
    keep = []
    n = len(genes)
    alns = (_lib.Alignment * n)(*[_aln_struct(g[0], g[1], keep) for g in genes])
    p = C.c_void_p()
    if sel is None:
        rc = L.pml_concatenate(n, alns, 0, None, C.byref(p))
    else:
        arr = (C.c_int * len(sel))(*sel)
        rc = L.pml_concatenate(n, alns, len(sel), arr, C.byref(p))
    if rc:
        raise PmlError(rc)
    txt = C.string_at(p).decode()
    L.pml_free(p)
    lines = txt.splitlines()
    return [l[1:] for l in lines[0::2]], lines[1::2]
