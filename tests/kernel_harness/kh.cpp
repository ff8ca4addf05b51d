// kh.cpp -- kernel harness (test infrastructure): thin extern "C" doors to the pml::launch_* functions of libpeprml.so, so that
// a test can hand ONE kernel its descriptors and compare what it wrote with a reference of that one operation.
//
// The harness owns no device memory: every pointer is the data_ptr() of a tensor the test allocated, and the test lists those
// tensors as `regions` {base, bytes}.  Descriptors arrive in HOST memory; every pointer in them, with the extent the kernel will
// touch behind it, is checked against the regions BEFORE anything is launched, together with the invariants the engine keeps
// (mpad a multiple of 32, kind / mode / flag combinations it emits, ticket tables as it builds them).  A mistake in a test is a
// negative return code and a message (kh_last_error), never an out-of-bounds access on the device.  Only then are the
// descriptors copied into the test's descriptor tensor and the kernel launched on the given stream; the door synchronises the
// stream and returns the hipError_t (>= 0).
#include "../../pepr_amd/csrc/kernels.h"

#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <set>
#include <vector>

using namespace pml;

namespace {

struct Region { unsigned long long base, bytes; };
char g_err[512] = "";
unsigned g_launch = 0;       // Newton exchange tags: (launch number << 10), unique per launch of this process

int refuse(int code, const char *fmt, ...) {
    va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof g_err, fmt, ap); va_end(ap);
    return code;
}

struct Check {
    const Region *r; int n;
    // [p, p + bytes) lies inside one region and p is aligned
    bool in(const void *p, size_t bytes, size_t align = 8) const {
        const unsigned long long a = (unsigned long long)(uintptr_t)p;
        if (p == nullptr || bytes == 0 || a % align != 0) return false;
        for (int i = 0; i < n; ++i) if (a >= r[i].base && a + bytes <= r[i].base + r[i].bytes && a + bytes > a) return true;
        return false;
    }
};
enum { KH_EPTR = -2, KH_ESHAPE = -3, KH_EKIND = -4, KH_ETICKET = -5, KH_EGAVEUP = -6 };
#define NEED(cond, code, ...) do { if (!(cond)) return refuse(code, __VA_ARGS__); } while (0)

int finish(hipStream_t s) {
    hipError_t e = hipGetLastError();
    const hipError_t e2 = hipStreamSynchronize(s);
    if (e == hipSuccess) e = e2;
    if (e != hipSuccess) refuse((int)e, "hip: %s", hipGetErrorString(e));
    return (int)e;
}
template <class T>
int upload(const Check &ck, void *dev, const T *host, int n, hipStream_t s, const char *what) {
    NEED(n > 0 && host != nullptr, KH_ESHAPE, "%s: empty descriptor list", what);
    NEED(ck.in(dev, sizeof(T) * (size_t)n), KH_EPTR, "%s: descriptor tensor too small for %d entries", what, n);
    const hipError_t e = hipMemcpyAsync(dev, host, sizeof(T) * (size_t)n, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return refuse((int)e, "hip: %s", hipGetErrorString(e));
    return 0;
}

struct Field { const char *st, *f; size_t off; };
#define F(S, f) {#S, #f, offsetof(S, f)}
const Field g_fields[] = {
    F(ModelDev, eval), F(ModelDev, U), F(ModelDev, Uinv), F(ModelDev, pi), F(ModelDev, UinvT),
    F(PmatReq, t), F(PmatReq, rates), F(PmatReq, kind), F(PmatReq, pad), F(PmatReq, tp), F(PmatReq, md),
    F(OpSide, p0), F(OpSide, p1), F(OpSide, p2), F(OpSide, t0), F(OpSide, t1), F(OpSide, t2), F(OpSide, f),
    F(NvOp, out), F(NvOp, l), F(NvOp, r), F(NvOp, out_scl), F(NvOp, l_scl), F(NvOp, r_scl), F(NvOp, pl), F(NvOp, pr), F(NvOp, mpad),
    F(NvOp, flags), F(NvOp, mode), F(NvOp, pad), F(NvOp, aux),
    F(GeneRun, op_begin), F(GeneRun, op_end),
    F(ReduceReq, patlnl), F(ReduceReq, weight), F(ReduceReq, out), F(ReduceReq, mpad), F(ReduceReq, pad),
    F(NewtonReq, sumtab), F(NewtonReq, weight), F(NewtonReq, scl), F(NewtonReq, rates), F(NewtonReq, t0), F(NewtonReq, tol), F(NewtonReq, out),
    F(NewtonReq, sync), F(NewtonReq, md), F(NewtonReq, tag_base), F(NewtonReq, pad0), F(NewtonReq, t_dev0), F(NewtonReq, t_dev1),
    F(NewtonReq, patlnl), F(NewtonReq, mpad), F(NewtonReq, max_iter), F(NewtonReq, ticket0), F(NewtonReq, pad),
    F(NewtonCtl, ticket), F(NewtonCtl, done), F(NewtonCtl, abort), F(NewtonCtl, odone), F(NewtonCtl, pad), F(NewtonCtl, oticket), F(NewtonCtl, dbg),
    F(NewtonCtl, n_requests), F(NewtonCtl, n_evals),
    F(G20Req, table), F(G20Req, cnt), F(G20Req, weight), F(G20Req, w), F(G20Req, out), F(G20Req, patlnl), F(G20Req, mpad), F(G20Req, pad),
    F(ShReq, l0), F(ShReq, l1), F(ShReq, l2), F(ShReq, site2pat), F(ShReq, out), F(ShReq, seed), F(ShReq, nsites), F(ShReq, nboot),
    F(GatherSeg, src), F(GatherSeg, w), F(GatherSeg, dst), F(GatherSeg, dst_w), F(GatherSeg, rowmap), F(GatherSeg, src_mpad), F(GatherSeg, npat),
    F(GatherSeg, dst_mpad), F(GatherSeg, dst_off), F(GatherSeg, ntax_dst), F(GatherSeg, pad),
};
#undef F
struct Size { const char *st; size_t n; };
#define S(T) {#T, sizeof(T)}
const Size g_sizes[] = {S(ModelDev), S(PmatReq), S(OpSide), S(NvOp), S(GeneRun), S(ReduceReq), S(NewtonReq), S(NewtonCtl), S(G20Req), S(ShReq), S(GatherSeg)};
#undef S

}  // namespace

extern "C" {

const char *kh_last_error() { return g_err; }
long kh_sizeof(const char *name) {
    for (const Size &s : g_sizes) if (!strcmp(s.st, name)) return (long)s.n;
    return -1;
}
long kh_offsetof(const char *name, const char *field) {
    for (const Field &f : g_fields) if (!strcmp(f.st, name) && !strcmp(f.f, field)) return (long)f.off;
    return -1;
}
// the layout constants the packers of tests/kh.py mirror
long kh_const(const char *name) {
    if (!strcmp(name, "PFRAG")) return PFRAG;
    if (!strcmp(name, "FRAG_STRIDE")) return FRAG_STRIDE;
    if (!strcmp(name, "TIPTAB_DOUBLES")) return TIPTAB_DOUBLES;
    if (!strcmp(name, "NEWTON_SYNC_DOUBLES")) return NEWTON_SYNC_DOUBLES;
    if (!strcmp(name, "NEWTON_MAX_SPLIT")) return NEWTON_MAX_SPLIT;
    if (!strcmp(name, "TILE_PAT")) return TILE_PAT;
    if (!strcmp(name, "NCODES")) return NCODES;
    return -1;
}
long kh_clv_doubles(int mpad) { return (long)clv_doubles(mpad); }
long kh_clv_index(int row, int p) { return (long)clv_index(row, p); }
int kh_newton_split(int mpad) { return newton_split(mpad); }
int kh_newton_slice(int mpad) { return newton_slice(mpad); }
int kh_newton_reg_form(int mpad) { return newton_reg_form(mpad) ? 1 : 0; }

int kh_pmat(const Region *regs, int nregs, const ModelDev *model, const PmatReq *reqs, int n, int per_request, PmatReq *dev_reqs,
            double *frags, hipStream_t s) {
    const Check ck{regs, nregs};
    NEED(n > 0 && n <= 1 << 16, KH_ESHAPE, "pmat: n = %d", n);
    NEED(per_request || ck.in(model, sizeof(ModelDev)), KH_EPTR, "pmat: launch model outside the regions");
    NEED(ck.in(frags, (size_t)n * FRAG_STRIDE * 8, 16), KH_EPTR, "pmat: output smaller than n x FRAG_STRIDE doubles");
    for (int i = 0; i < n; ++i) {
        NEED(reqs[i].kind >= PM_FRAGS && reqs[i].kind <= PM_TIPTABLE, KH_EKIND, "pmat: request %d kind %d", i, reqs[i].kind);
        NEED(reqs[i].tp == nullptr || ck.in(reqs[i].tp, 8), KH_EPTR, "pmat: request %d tp outside the regions", i);
        NEED(!per_request || ck.in(reqs[i].md, sizeof(ModelDev)), KH_EPTR, "pmat: request %d names no model", i);
    }
    if (int rc = upload(ck, dev_reqs, reqs, n, s, "pmat")) return rc;
    launch_pmat(per_request ? nullptr : model, dev_reqs, frags, n, s, per_request != 0);
    return finish(s);
}

int kh_eigfrags(const Region *regs, int nregs, const ModelDev *models, int n, double *frags2, hipStream_t s) {
    const Check ck{regs, nregs};
    NEED(n > 0 && n <= 4096, KH_ESHAPE, "eigfrags: n = %d", n);
    NEED(ck.in(models, sizeof(ModelDev) * (size_t)n), KH_EPTR, "eigfrags: models outside the regions");
    NEED(ck.in(frags2, (size_t)n * 2 * PFRAG * 8), KH_EPTR, "eigfrags: output smaller than n x 2 PFRAG doubles");
    if (n == 1) launch_eigfrags(models, frags2, s); else launch_eigfrags_n(models, frags2, n, s);
    return finish(s);
}

// tip codes index the 23-row tables: read back and checked
static int check_codes(const void *dev, int mpad, int i, const char *which) {
    std::vector<unsigned char> h((size_t)mpad);
    const hipError_t e = hipMemcpy(h.data(), dev, (size_t)mpad, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return refuse((int)e, "hip: %s", hipGetErrorString(e));
    for (int p = 0; p < mpad; ++p) NEED(h[p] < NCODES, KH_ESHAPE, "oplist: op %d %s code %d at pattern %d", i, which, (int)h[p], p);
    return 0;
}

// one side of an operation: every extent the kernel reads for that kind
static int check_side(const Check &ck, const OpSide &sd, int kind, const int *scl, bool chained_in, int mode, int mpad, int i, const char *which) {
    const size_t tab = (size_t)TIPTAB_DOUBLES * 8;
    if (kind == SK_CLV) {
        if (chained_in) return 0;          // taken from the registers: the kernel touches neither p0 nor the counts
        NEED(ck.in(sd.p0, clv_doubles(mpad) * 8, 16), KH_EPTR, "oplist: op %d %s CLV smaller than clv_doubles(mpad)", i, which);
        NEED(ck.in(scl, (size_t)mpad * 4), KH_EPTR, "oplist: op %d %s counts smaller than mpad ints", i, which);
        return 0;
    }
    NEED(scl == nullptr, KH_EKIND, "oplist: op %d %s: counts on a side that is no CLV", i, which);
    NEED(ck.in(sd.p0, (size_t)mpad, 2), KH_EPTR, "oplist: op %d %s codes smaller than mpad", i, which);
    if (int rc = check_codes(sd.p0, mpad, i, which)) return rc;
    if (kind == SK_TIP) return 0;
    NEED(ck.in(sd.p1, (size_t)mpad, 2), KH_EPTR, "oplist: op %d %s second codes smaller than mpad", i, which);
    if (int rc = check_codes(sd.p1, mpad, i, which)) return rc;
    NEED(ck.in(sd.t0, tab, 16) && ck.in(sd.t1, tab, 16), KH_EPTR, "oplist: op %d %s tip tables", i, which);
    if (kind == SK_CHERRY) return 0;
    NEED(ck.in(sd.p2, (size_t)mpad, 2), KH_EPTR, "oplist: op %d %s third codes smaller than mpad", i, which);
    if (int rc = check_codes(sd.p2, mpad, i, which)) return rc;
    NEED(ck.in(sd.t2, tab, 16), KH_EPTR, "oplist: op %d %s third tip table", i, which);
    NEED(ck.in(sd.f, (size_t)PFRAG * 8, 16), KH_EPTR, "oplist: op %d %s inner fragment set", i, which);
    (void)mode;
    return 0;
}

// variants 1 (chained = 0) and 11 (chained = 1) of k_oplist, no fused Newton (ctl = null)
int kh_oplist(const Region *regs, int nregs, const NvOp *ops, int nops, const GeneRun *runs, int nruns, int chained, NvOp *dev_ops,
              GeneRun *dev_runs, hipStream_t s) {
    const Check ck{regs, nregs};
    NEED(nops > 0 && nops <= 4096 && nruns > 0 && nruns <= 1024, KH_ESHAPE, "oplist: %d ops, %d runs", nops, nruns);
    int max_mpad = 0; bool any_pitch = false;
    std::vector<char> covered(nops, 0);
    for (int g = 0; g < nruns; ++g) {
        const GeneRun &run = runs[g];
        NEED(run.op_begin >= 0 && run.op_begin < run.op_end && run.op_end <= nops, KH_ESHAPE, "oplist: run %d = [%d, %d)", g, run.op_begin, run.op_end);
        const int mpad = ops[run.op_begin].mpad;
        NEED(mpad > 0 && mpad % 32 == 0 && mpad <= 1 << 22, KH_ESHAPE, "oplist: run %d mpad %d is no multiple of 32", g, mpad);
        max_mpad = mpad > max_mpad ? mpad : max_mpad;
        bool have_x = false;               // the previous operation of the run was a newview: its result is in the registers
        for (int i = run.op_begin; i < run.op_end; ++i) {
            const NvOp &op = ops[i];
            NEED(!covered[i], KH_ESHAPE, "oplist: op %d belongs to two runs", i);
            covered[i] = 1;
            NEED(op.mpad == mpad, KH_ESHAPE, "oplist: op %d mpad %d differs from its run's %d", i, op.mpad, mpad);
            NEED(op.mode >= MODE_NEWVIEW && op.mode <= MODE_EVALUATE_CAT, KH_EKIND, "oplist: op %d mode %d", i, op.mode);
            const int known = 15 | OPF_NT_STORE | OPF_CHAIN_L | OPF_CHAIN_R | OPF_NO_STORE;
            NEED((op.flags & ~known) == 0, KH_EKIND, "oplist: op %d flags %#x (fused Newton tails are not driven from here)", i, op.flags);
            NEED(op.aux == nullptr, KH_EKIND, "oplist: op %d carries a Newton request", i);
            const int lk = op.flags & 3, rk = (op.flags >> 2) & 3;
            const bool chL = op.flags & OPF_CHAIN_L, chR = op.flags & OPF_CHAIN_R, nost = op.flags & OPF_NO_STORE;
            NEED(!(chL || chR || nost) || chained, KH_EKIND, "oplist: op %d chaining flags in an unchained launch", i);
            NEED(!(chL && chR), KH_EKIND, "oplist: op %d chained on both sides", i);
            NEED(!chL || (have_x && lk == SK_CLV), KH_EKIND, "oplist: op %d OPF_CHAIN_L without a newview result in front of it", i);
            NEED(!chR || (have_x && rk == SK_CLV && op.mode >= MODE_EVALUATE), KH_EKIND, "oplist: op %d OPF_CHAIN_R is for evaluate tails behind a newview", i);
            if (nost) {                    // the engine sets it on a newview whose result the NEXT operation of the run takes from the registers
                NEED(op.mode == MODE_NEWVIEW && i + 1 < run.op_end && (ops[i + 1].flags & (OPF_CHAIN_L | OPF_CHAIN_R)), KH_EKIND,
                     "oplist: op %d OPF_NO_STORE but nothing consumes it", i);
            }
            NEED(!(op.flags & OPF_NT_STORE) || op.mode == MODE_NEWVIEW, KH_EKIND, "oplist: op %d OPF_NT_STORE on a tail", i);
            any_pitch = any_pitch || lk == SK_PITCH || rk == SK_PITCH;
            if (int rc = check_side(ck, op.l, lk, op.l_scl, chL, op.mode, mpad, i, "left")) return rc;
            if (int rc = check_side(ck, op.r, rk, op.r_scl, chR, op.mode, mpad, i, "right")) return rc;
            NEED(ck.in(op.pr, (size_t)PFRAG * 8, 16), KH_EPTR, "oplist: op %d right fragment set", i);
            if (op.mode >= MODE_EVALUATE) NEED(op.pl == op.pr, KH_EKIND, "oplist: op %d evaluate takes pl = pr (one PM_FRAGS_PI set)", i);
            else NEED(ck.in(op.pl, (size_t)PFRAG * 8, 16), KH_EPTR, "oplist: op %d left fragment set", i);
            if (op.mode == MODE_NEWVIEW || op.mode == MODE_SUMTABLE) {
                // (a newview under OPF_NO_STORE writes nothing, but the engine still names its slot: so does a test)
                NEED(ck.in(op.out, clv_doubles(mpad) * 8, 16), KH_EPTR, "oplist: op %d output smaller than clv_doubles(mpad)", i);
                NEED(ck.in(op.out_scl, (size_t)mpad * 4), KH_EPTR, "oplist: op %d output counts", i);
            } else if (op.mode == MODE_EVALUATE) {
                NEED(ck.in(op.out, (size_t)mpad * 8, 16), KH_EPTR, "oplist: op %d per-pattern lnL smaller than mpad", i);
                NEED(op.out_scl == nullptr, KH_EKIND, "oplist: op %d evaluate writes no counts", i);
            } else {
                NEED(ck.in(op.out, (size_t)mpad * 8 * NCAT, 16), KH_EPTR, "oplist: op %d table slice smaller than 4 x mpad", i);
                NEED(ck.in(op.out_scl, (size_t)mpad * 4), KH_EPTR, "oplist: op %d table counts", i);
            }
            have_x = op.mode == MODE_NEWVIEW || (have_x && op.mode >= MODE_EVALUATE);     // a sumtable leaves its own tile there
        }
    }
    for (int i = 0; i < nops; ++i) NEED(covered[i], KH_ESHAPE, "oplist: op %d belongs to no run", i);
    if (int rc = upload(ck, dev_ops, ops, nops, s, "oplist ops")) return rc;
    if (int rc = upload(ck, dev_runs, runs, nruns, s, "oplist runs")) return rc;
    launch_oplist(dev_ops, dev_runs, nruns, max_mpad, any_pitch, chained != 0, s, nullptr);
    return finish(s);
}

int kh_reduce(const Region *regs, int nregs, const ReduceReq *reqs, int n, ReduceReq *dev_reqs, hipStream_t s) {
    const Check ck{regs, nregs};
    NEED(n > 0 && n <= 65535, KH_ESHAPE, "reduce: n = %d", n);
    for (int i = 0; i < n; ++i) {
        NEED(reqs[i].mpad > 0, KH_ESHAPE, "reduce: request %d mpad %d", i, reqs[i].mpad);
        NEED(ck.in(reqs[i].patlnl, (size_t)reqs[i].mpad * 8) && ck.in(reqs[i].weight, (size_t)reqs[i].mpad * 8), KH_EPTR, "reduce: request %d inputs", i);
        NEED(ck.in(reqs[i].out, 8), KH_EPTR, "reduce: request %d output", i);
    }
    if (int rc = upload(ck, dev_reqs, reqs, n, s, "reduce")) return rc;
    launch_reduce(dev_reqs, n, s);
    return finish(s);
}

// k_newton in its split form (seq = 0: `tickets` = one entry per (request, slice), register-form requests first, as engine.cpp
// builds the table) or its no-exchange form (seq = 1: one entry per request).  The exchange tags are set here (unique per
// launch), the control block is zeroed on the launch stream, and a give-up (which a valid launch never produces) is an error.
int kh_newton(const Region *regs, int nregs, const ModelDev *model, NewtonReq *reqs, int nreq, const int *tickets, int nreg, int nstream, int seq,
              NewtonReq *dev_reqs, int *dev_tickets, NewtonCtl *ctl, hipStream_t s) {
    const Check ck{regs, nregs};
    NEED(nreq > 0 && nreq <= 4096 && nreg >= 0 && nstream >= 0 && nreg + nstream > 0, KH_ESHAPE, "newton: %d requests, %d + %d tickets", nreq, nreg, nstream);
    NEED(ck.in(model, sizeof(ModelDev)), KH_EPTR, "newton: model outside the regions");
    NEED(ck.in(ctl, sizeof(NewtonCtl)), KH_EPTR, "newton: control block outside the regions");
    ++g_launch;
    std::set<const double *> syncs;
    for (int i = 0; i < nreq; ++i) {
        NewtonReq &r = reqs[i];
        NEED(r.mpad > 0 && r.mpad % 32 == 0 && r.mpad <= 1 << 22, KH_ESHAPE, "newton: request %d mpad %d is no multiple of 32", i, r.mpad);
        NEED(ck.in(r.sumtab, clv_doubles(r.mpad) * 8), KH_EPTR, "newton: request %d sumtable smaller than clv_doubles(mpad)", i);
        NEED(ck.in(r.weight, (size_t)r.mpad * 8) && ck.in(r.scl, (size_t)r.mpad * 4, 4), KH_EPTR, "newton: request %d weights / counts", i);
        NEED(ck.in(r.out, 32) && ck.in(r.md, sizeof(ModelDev)), KH_EPTR, "newton: request %d output / model", i);
        NEED(ck.in(r.sync, (size_t)NEWTON_SYNC_DOUBLES * 8) && syncs.insert(r.sync).second, KH_EPTR, "newton: request %d needs an exchange block of its own", i);
        NEED((r.t_dev0 == nullptr) == (r.t_dev1 == nullptr) && (r.t_dev0 == nullptr || (ck.in(r.t_dev0, 8) && ck.in(r.t_dev1, 8))), KH_EPTR, "newton: request %d t_dev", i);
        NEED(r.patlnl == nullptr || ck.in(r.patlnl, (size_t)r.mpad * 8), KH_EPTR, "newton: request %d patlnl", i);
        NEED(r.max_iter >= 0 && r.max_iter <= 64 && r.tol > 0.0 && r.t0 == r.t0, KH_ESHAPE, "newton: request %d iteration settings", i);
        r.tag_base = g_launch << 10; r.pad0 = 0; r.pad = 0;
    }
    // the ticket table: requests in order, register form first; request i holds newton_split(mpad) consecutive tickets from ticket0
    int cur = 0, seen = 0;
    for (int pass = 0; pass < 2; ++pass) {
        const int base = pass == 0 ? 0 : nreg;
        for (int i = 0; i < nreq; ++i) {
            if (newton_reg_form(reqs[i].mpad) != (pass == 0)) continue;
            const int S = seq ? 1 : newton_split(reqs[i].mpad);
            NEED(seq || reqs[i].ticket0 == cur - base, KH_ETICKET, "newton: request %d ticket0 %d, table says %d", i, reqs[i].ticket0, cur - base);
            for (int k = 0; k < S; ++k, ++cur) NEED(cur < nreg + nstream && tickets[cur] == i, KH_ETICKET, "newton: ticket %d does not name request %d", cur, i);
            ++seen;
        }
        NEED(cur == (pass == 0 ? nreg : nreg + nstream), KH_ETICKET, "newton: %d tickets of form %d, expected %d", cur - base, pass, pass == 0 ? nreg : nstream);
    }
    NEED(seen == nreq, KH_ETICKET, "newton: requests missing from the table");
    if (int rc = upload(ck, dev_reqs, reqs, nreq, s, "newton requests")) return rc;
    if (int rc = upload(ck, dev_tickets, tickets, nreg + nstream, s, "newton tickets")) return rc;
    hipError_t e = hipMemsetAsync(ctl, 0, sizeof(NewtonCtl), s);
    if (e != hipSuccess) return refuse((int)e, "hip: %s", hipGetErrorString(e));
    if (seq) launch_newton_seq(model, dev_reqs, dev_tickets, nreg, nstream, ctl, s);
    else launch_newton(model, dev_reqs, dev_tickets, nreg, nstream, ctl, s);
    if (int rc = finish(s)) return rc;
    NewtonCtl h;
    e = hipMemcpy(&h, ctl, sizeof h, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return refuse((int)e, "hip: %s", hipGetErrorString(e));
    NEED(h.abort == 0, KH_EGAVEUP, "newton: an exchange gave up (slice %d of %d, evaluation %d)", h.dbg[1], h.dbg[2], h.dbg[3]);
    return 0;
}

int kh_g20(const Region *regs, int nregs, const G20Req *reqs, int n, G20Req *dev_reqs, hipStream_t s) {
    const Check ck{regs, nregs};
    NEED(n > 0 && n <= 65535, KH_ESHAPE, "g20: n = %d", n);
    for (int i = 0; i < n; ++i) {
        const G20Req &r = reqs[i];
        NEED(r.mpad > 0, KH_ESHAPE, "g20: request %d mpad %d", i, r.mpad);
        NEED(ck.in(r.table, (size_t)r.mpad * 8 * G20_RATES) && ck.in(r.cnt, (size_t)r.mpad * 4 * (G20_RATES / 4), 4) && ck.in(r.weight, (size_t)r.mpad * 8),
             KH_EPTR, "g20: request %d inputs", i);
        NEED(ck.in(r.out, 8) && (r.patlnl == nullptr || ck.in(r.patlnl, (size_t)r.mpad * 8)), KH_EPTR, "g20: request %d outputs", i);
    }
    if (int rc = upload(ck, dev_reqs, reqs, n, s, "g20")) return rc;
    launch_g20(dev_reqs, n, s);
    return finish(s);
}

// npat[i]: length of request i's three per-pattern vectors; its site -> pattern map is read back and checked against it
int kh_sh(const Region *regs, int nregs, const ShReq *reqs, const int *npat, int n, ShReq *dev_reqs, hipStream_t s) {
    const Check ck{regs, nregs};
    NEED(n > 0 && n <= 65535, KH_ESHAPE, "sh: n = %d", n);
    std::vector<int> map;
    for (int i = 0; i < n; ++i) {
        const ShReq &r = reqs[i];
        NEED(r.nsites > 0 && r.nsites <= 1 << 20 && r.nboot >= 0 && r.nboot <= 100000 && npat[i] > 0, KH_ESHAPE, "sh: request %d sizes", i);
        const size_t vb = (size_t)npat[i] * 8;
        NEED(ck.in(r.l0, vb) && ck.in(r.l1, vb) && ck.in(r.l2, vb) && ck.in(r.site2pat, (size_t)r.nsites * 4, 4) && ck.in(r.out, 8), KH_EPTR, "sh: request %d pointers", i);
        map.resize(r.nsites);
        const hipError_t e = hipMemcpy(map.data(), r.site2pat, (size_t)r.nsites * 4, hipMemcpyDeviceToHost);
        if (e != hipSuccess) return refuse((int)e, "hip: %s", hipGetErrorString(e));
        for (int j = 0; j < r.nsites; ++j) NEED(map[j] >= 0 && map[j] < npat[i], KH_ESHAPE, "sh: request %d site %d maps to pattern %d", i, j, map[j]);
    }
    if (int rc = upload(ck, dev_reqs, reqs, n, s, "sh")) return rc;
    launch_sh(dev_reqs, n, s);
    return finish(s);
}

// src_rows[i]: taxa (rows of src_mpad codes) of segment i's source; its row map is read back and checked against it
int kh_gather(const Region *regs, int nregs, const GatherSeg *segs, const int *src_rows, int n, GatherSeg *dev_segs, hipStream_t s) {
    const Check ck{regs, nregs};
    NEED(n > 0 && n <= 65535, KH_ESHAPE, "gather: n = %d", n);
    int max_npat = 0;
    std::vector<int> map;
    for (int i = 0; i < n; ++i) {
        const GatherSeg &g = segs[i];
        NEED(g.npat > 0 && g.npat <= g.src_mpad && g.dst_off >= 0 && g.dst_off + g.npat <= g.dst_mpad && g.ntax_dst > 0 && g.ntax_dst <= 1 << 16 && src_rows[i] > 0,
             KH_ESHAPE, "gather: segment %d sizes", i);
        NEED(ck.in(g.src, (size_t)src_rows[i] * g.src_mpad, 1) && ck.in(g.w, (size_t)g.npat * 8) && ck.in(g.dst, (size_t)g.ntax_dst * g.dst_mpad, 1) &&
             ck.in(g.dst_w, (size_t)g.dst_mpad * 8) && ck.in(g.rowmap, (size_t)g.ntax_dst * 4, 4), KH_EPTR, "gather: segment %d pointers", i);
        map.resize(g.ntax_dst);
        const hipError_t e = hipMemcpy(map.data(), g.rowmap, (size_t)g.ntax_dst * 4, hipMemcpyDeviceToHost);
        if (e != hipSuccess) return refuse((int)e, "hip: %s", hipGetErrorString(e));
        for (int t = 0; t < g.ntax_dst; ++t) NEED(map[t] >= -1 && map[t] < src_rows[i], KH_ESHAPE, "gather: segment %d row map entry %d = %d", i, t, map[t]);
        max_npat = g.npat > max_npat ? g.npat : max_npat;
    }
    if (int rc = upload(ck, dev_segs, segs, n, s, "gather")) return rc;
    launch_gather(dev_segs, n, max_npat, s);
    return finish(s);
}

}  // extern "C"
