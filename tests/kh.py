"""Python side of the kernel harness (tests/kernel_harness/kh.cpp): ctypes mirrors of the descriptor structs of
pepr_amd/csrc/kernels.h, packers for the device layouts, and a `Dev` object that owns the torch tensors a test hands to a
kernel and lists them to the harness as the only memory a descriptor may point into.

A refusal of the harness (bad pointer, bad shape, a kind / flag combination the engine does not emit) is a KhError."""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "kernel_harness", "libkh.so")

NS, NCAT, CLV_ROWS, NCODES, TILE_PAT, TIPTAB_KK = 20, 4, 80, 23, 128, 6
PFRAG = NCAT * 25 * 16
TIPTAB_DOUBLES = NCAT * NCODES * 4 * TIPTAB_KK
FRAG_STRIDE = TIPTAB_DOUBLES
NEWTON_MAX_SPLIT = 64
NEWTON_SYNC_DOUBLES = 2 * NEWTON_MAX_SPLIT * 6
PM_FRAGS, PM_FRAGS_PI, PM_TIPTABLE = 0, 1, 2
SK_CLV, SK_TIP, SK_CHERRY, SK_PITCH = 0, 1, 2, 3
OPF_NT_STORE, OPF_CHAIN_L, OPF_CHAIN_R, OPF_NO_STORE = 16, 32, 64, 128
MODE_NEWVIEW, MODE_SUMTABLE, MODE_EVALUATE, MODE_EVALUATE_CAT = 0, 1, 2, 3
LOG_2_256 = 256.0 * np.log(2.0)

_p, _d, _i = C.c_void_p, C.c_double, C.c_int


class ModelDev(C.Structure):
    _fields_ = [("eval", _d * 20), ("U", _d * 400), ("Uinv", _d * 400), ("pi", _d * 20), ("UinvT", _d * 400)]


class PmatReq(C.Structure):
    _fields_ = [("t", _d), ("rates", _d * 4), ("kind", _i), ("pad", _i), ("tp", _p), ("md", _p)]


class OpSide(C.Structure):
    _fields_ = [("p0", _p), ("p1", _p), ("p2", _p), ("t0", _p), ("t1", _p), ("t2", _p), ("f", _p)]


class NvOp(C.Structure):
    _fields_ = [("out", _p), ("l", OpSide), ("r", OpSide), ("out_scl", _p), ("l_scl", _p), ("r_scl", _p), ("pl", _p), ("pr", _p),
                ("mpad", _i), ("flags", _i), ("mode", _i), ("pad", _i), ("aux", _p)]


class GeneRun(C.Structure):
    _fields_ = [("op_begin", _i), ("op_end", _i)]


class ReduceReq(C.Structure):
    _fields_ = [("patlnl", _p), ("weight", _p), ("out", _p), ("mpad", _i), ("pad", _i)]


class NewtonReq(C.Structure):
    _fields_ = [("sumtab", _p), ("weight", _p), ("scl", _p), ("rates", _d * 4), ("t0", _d), ("tol", _d), ("out", _p), ("sync", _p),
                ("md", _p), ("tag_base", C.c_uint), ("pad0", C.c_uint), ("t_dev0", _p), ("t_dev1", _p), ("patlnl", _p),
                ("mpad", _i), ("max_iter", _i), ("ticket0", _i), ("pad", _i)]


class NewtonCtl(C.Structure):
    _fields_ = [("ticket", _i * 2), ("done", _i * 2), ("abort", _i), ("odone", _i), ("pad", _i * 2), ("oticket", _i * 8), ("dbg", _i * 8),
                ("n_requests", C.c_ulonglong), ("n_evals", C.c_ulonglong)]


class G20Req(C.Structure):
    _fields_ = [("table", _p), ("cnt", _p), ("weight", _p), ("w", _d * 20), ("out", _p), ("patlnl", _p), ("mpad", _i), ("pad", _i)]


class ShReq(C.Structure):
    _fields_ = [("l0", _p), ("l1", _p), ("l2", _p), ("site2pat", _p), ("out", _p), ("seed", C.c_ulonglong), ("nsites", _i), ("nboot", _i)]


class GatherSeg(C.Structure):
    _fields_ = [("src", _p), ("w", _p), ("dst", _p), ("dst_w", _p), ("rowmap", _p), ("src_mpad", _i), ("npat", _i), ("dst_mpad", _i),
                ("dst_off", _i), ("ntax_dst", _i), ("pad", _i)]


class Region(C.Structure):
    _fields_ = [("base", C.c_ulonglong), ("bytes", C.c_ulonglong)]


MIRRORS = {c.__name__: c for c in (ModelDev, PmatReq, OpSide, NvOp, GeneRun, ReduceReq, NewtonReq, NewtonCtl, G20Req, ShReq, GatherSeg)}
CONSTANTS = {"PFRAG": PFRAG, "FRAG_STRIDE": FRAG_STRIDE, "TIPTAB_DOUBLES": TIPTAB_DOUBLES, "NEWTON_SYNC_DOUBLES": NEWTON_SYNC_DOUBLES,
             "NEWTON_MAX_SPLIT": NEWTON_MAX_SPLIT, "TILE_PAT": TILE_PAT, "NCODES": NCODES}


class KhError(RuntimeError):
    pass


_lib = None


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(LIB_PATH)
        L.kh_last_error.restype = C.c_char_p
        for f in ("kh_sizeof", "kh_offsetof", "kh_const", "kh_clv_doubles", "kh_clv_index"):
            getattr(L, f).restype = C.c_long
        L.kh_sizeof.argtypes = [C.c_char_p]; L.kh_offsetof.argtypes = [C.c_char_p, C.c_char_p]; L.kh_const.argtypes = [C.c_char_p]
        R = C.POINTER(Region)
        L.kh_pmat.argtypes = [R, _i, _p, C.POINTER(PmatReq), _i, _i, _p, _p, _p]
        L.kh_eigfrags.argtypes = [R, _i, _p, _i, _p, _p]
        L.kh_oplist.argtypes = [R, _i, C.POINTER(NvOp), _i, C.POINTER(GeneRun), _i, _i, _p, _p, _p]
        L.kh_reduce.argtypes = [R, _i, C.POINTER(ReduceReq), _i, _p, _p]
        L.kh_newton.argtypes = [R, _i, _p, C.POINTER(NewtonReq), _i, C.POINTER(_i), _i, _i, _i, _p, _p, _p, _p]
        L.kh_g20.argtypes = [R, _i, C.POINTER(G20Req), _i, _p, _p]
        L.kh_sh.argtypes = [R, _i, C.POINTER(ShReq), C.POINTER(_i), _i, _p, _p]
        L.kh_gather.argtypes = [R, _i, C.POINTER(GatherSeg), C.POINTER(_i), _i, _p, _p]
        _lib = L
    return _lib


# ---------------------------------------------------------------------------------------------------------------------------
# layouts (numpy, host side)
# ---------------------------------------------------------------------------------------------------------------------------
def clv_doubles(mpad):
    return ((mpad + TILE_PAT - 1) // TILE_PAT) * TILE_PAT * CLV_ROWS


def clv_index(row, p):
    """tiled CLV / sumtable: element (row, p) at ((p >> 7) * 80 + row) * 128 + (p & 127); row, p may be arrays"""
    return ((p >> 7) * CLV_ROWS + row) * TILE_PAT + (p & (TILE_PAT - 1))


def clv_pack(a, mpad, fill=1.0):
    """a[80][npat] -> the tiled buffer of clv_doubles(mpad) doubles; columns npat.. (padding) hold `fill`"""
    a = np.asarray(a, np.float64)
    full = np.full((CLV_ROWS, mpad), fill)
    full[:, :a.shape[1]] = a
    out = np.zeros(clv_doubles(mpad))
    out[clv_index(np.arange(CLV_ROWS)[:, None], np.arange(mpad)[None, :])] = full
    return out


def clv_unpack(flat, mpad):
    return np.asarray(flat)[clv_index(np.arange(CLV_ROWS)[:, None], np.arange(mpad)[None, :])]


def _frag_map():
    """fragment order: element 4k+i of fragment (c, st, kk) = M_c[4 st + i][4 kk + k] -> (c, row, col) per flat index"""
    idx = np.arange(PFRAG)
    e, f = idx & 15, idx >> 4
    c, st, kk = f // 25, (f % 25) // 5, f % 5
    return c, 4 * st + (e & 3), 4 * kk + (e >> 2)


def frag_pack(m):
    """m[4][20][20] -> PFRAG doubles in MFMA A-fragment order"""
    c, r, k = _frag_map()
    return np.ascontiguousarray(np.asarray(m, np.float64)[c, r, k])


def frag_unpack(flat):
    c, r, k = _frag_map()
    m = np.zeros((NCAT, NS, NS))
    m[c, r, k] = np.asarray(flat)[:PFRAG]
    return m


def tiptab_unpack(flat):
    """T[c][code][q][kk] (kk padded to 6) -> t[c][code][s = 4 kk + q], and the padding entries"""
    t = np.asarray(flat)[:TIPTAB_DOUBLES].reshape(NCAT, NCODES, 4, TIPTAB_KK)
    return t[..., :5].transpose(0, 1, 3, 2).reshape(NCAT, NCODES, NS), t[..., 5]


def tiptab_pack(t):
    """t[c][code][s] -> the device table"""
    out = np.zeros((NCAT, NCODES, 4, TIPTAB_KK))
    out[..., :5] = np.asarray(t, np.float64).reshape(NCAT, NCODES, 5, 4).transpose(0, 1, 3, 2)
    return out.reshape(-1)


def code_sets():
    """states of the 23 tip codes: 0..19 single, 20 = N|D, 21 = Q|E, 22 = every state -> indicator [23][20]"""
    ind = np.zeros((NCODES, NS))
    ind[np.arange(20), np.arange(20)] = 1
    ind[20, [2, 3]] = 1
    ind[21, [5, 6]] = 1
    ind[22, :] = 1
    return ind


def newton_split(mpad):
    n = (mpad + 127) // 128
    return min(max(n, 1), NEWTON_MAX_SPLIT)


def newton_slice(mpad):
    return 128 if mpad <= 128 * NEWTON_MAX_SPLIT else ((mpad // 32 + newton_split(mpad) - 1) // newton_split(mpad)) * 32


def newton_reg_form(mpad):
    return newton_slice(mpad) <= 128


def newton_tickets(mpads, seq=False):
    """engine.cpp's ticket table: (request, slice) in request order, register-form requests first, then the streaming ones; ticket0
    relative to the request's kernel.  SEQ form: one entry per request.  -> (tickets, ticket0 per request, nreg, nstream)"""
    tickets, t0, nreg = [], [0] * len(mpads), 0
    for form in (True, False):
        for i, m in enumerate(mpads):
            if newton_reg_form(m) != form:
                continue
            t0[i] = len(tickets) - (0 if form else nreg)
            tickets += [i] * (1 if seq else newton_split(m))
        if form:
            nreg = len(tickets)
    return tickets, t0, nreg, len(tickets) - nreg


def model_struct(pi):
    """the eigensystem the engine hands the kernels (synth._eig of the normalised frequencies)"""
    from pepr_amd import synth
    pi = np.asarray(pi, np.float64) / np.sum(pi)
    lam, U, Uinv = synth._eig(pi)
    m = ModelDev()
    m.eval[:] = lam.tolist(); m.U[:] = U.reshape(-1).tolist(); m.Uinv[:] = Uinv.reshape(-1).tolist()
    m.pi[:] = pi.tolist(); m.UinvT[:] = Uinv.T.reshape(-1).tolist()
    return m, (lam, U, Uinv, pi)


# ---------------------------------------------------------------------------------------------------------------------------
# device side
# ---------------------------------------------------------------------------------------------------------------------------
class Dev:
    """Owns the tensors of one test.  Every tensor made here is a region a descriptor may point into; nothing else is."""

    def __init__(self):
        import torch
        self.torch = torch
        self.device = torch.device("cuda:0")
        self.tensors = []
        self.stream = torch.cuda.current_stream(self.device).cuda_stream
        self.desc = self.zeros(1 << 20, np.uint8)        # descriptors of a launch are copied here

    def put(self, a, dtype=None):
        a = np.ascontiguousarray(a, dtype)
        assert a.dtype in (np.float64, np.int32, np.uint8) and a.size > 0
        t = self.torch.from_numpy(a).to(self.device)
        self.tensors.append(t)
        return t

    def zeros(self, n, dtype=np.float64):
        return self.put(np.zeros(n, dtype))

    def codes(self, a, mpad):
        """tip codes of one taxon, padded to mpad with the gap code"""
        a = np.asarray(a)
        assert a.ndim == 1 and len(a) <= mpad and a.min() >= 0 and a.max() < NCODES
        full = np.full(mpad, NCODES - 1, np.uint8)
        full[:len(a)] = a
        return self.put(full)

    def struct(self, s):
        return self.put(np.frombuffer(bytes(s), np.uint8).copy())

    def regions(self):
        r = (Region * len(self.tensors))()
        for i, t in enumerate(self.tensors):
            r[i].base = t.data_ptr(); r[i].bytes = t.numel() * t.element_size()
        return r, len(self.tensors)

    def _call(self, fn, *args):
        r, n = self.regions()
        rc = fn(r, n, *args)
        if rc != 0:
            raise KhError("%s -> %d: %s" % (fn.__name__, rc, lib().kh_last_error().decode()))

    def _desc_split(self, *sizes):
        off, out = 0, []
        for s in sizes:
            out.append(self.desc.data_ptr() + off)
            off += (s + 255) // 256 * 256
        assert off <= self.desc.numel()
        return out

    def pmat(self, reqs, model=None, per_request=False):
        arr = (PmatReq * len(reqs))(*reqs)
        frags = self.zeros(len(reqs) * FRAG_STRIDE)
        frags += 7.0        # stale content must not pass for a result
        self._call(lib().kh_pmat, model.data_ptr() if model is not None else None, arr, len(reqs), int(per_request), self.desc.data_ptr(),
                   frags.data_ptr(), self.stream)
        return frags.cpu().numpy().reshape(len(reqs), FRAG_STRIDE)

    def eigfrags(self, models, n):
        out = self.zeros(n * 2 * PFRAG)
        self._call(lib().kh_eigfrags, models.data_ptr(), n, out.data_ptr(), self.stream)
        return out

    def oplist(self, ops, runs, chained):
        a = (NvOp * len(ops))(*ops)
        g = (GeneRun * len(runs))(*[GeneRun(b, e) for b, e in runs])
        d_ops, d_runs = self._desc_split(C.sizeof(a), C.sizeof(g))
        self._call(lib().kh_oplist, a, len(ops), g, len(runs), int(chained), d_ops, d_runs, self.stream)

    def reduce(self, reqs):
        a = (ReduceReq * len(reqs))(*reqs)
        self._call(lib().kh_reduce, a, len(reqs), self.desc.data_ptr(), self.stream)

    def newton(self, model, reqs, seq=False):
        """sets ticket0 of every request and builds the ticket table as the engine does; ctl is zeroed by the harness"""
        tickets, t0, nreg, nstream = newton_tickets([r.mpad for r in reqs], seq)
        for r, k in zip(reqs, t0):
            r.ticket0 = k
        a = (NewtonReq * len(reqs))(*reqs)
        tk = (_i * len(tickets))(*tickets)
        d_req, d_tk, d_ctl = self._desc_split(C.sizeof(a), C.sizeof(tk), C.sizeof(NewtonCtl))
        self._call(lib().kh_newton, model.data_ptr(), a, len(reqs), tk, nreg, nstream, int(seq), d_req, d_tk, d_ctl, self.stream)

    def g20(self, reqs):
        a = (G20Req * len(reqs))(*reqs)
        self._call(lib().kh_g20, a, len(reqs), self.desc.data_ptr(), self.stream)

    def sh(self, reqs, npat):
        a = (ShReq * len(reqs))(*reqs)
        self._call(lib().kh_sh, a, (_i * len(npat))(*npat), len(reqs), self.desc.data_ptr(), self.stream)

    def gather(self, segs, src_rows):
        a = (GatherSeg * len(segs))(*segs)
        self._call(lib().kh_gather, a, (_i * len(src_rows))(*src_rows), len(segs), self.desc.data_ptr(), self.stream)
