// launch.cpp -- from a request's operations and tails to launches: run() builds the descriptors of one launch set in the
// staging block (LaunchBuilder), submits it (at once, or deferred and grouped inside a chained pass) and, unless chained,
// waits for it and deals with Newton requests whose exchange gave up; replay_plan() issues a recorded scoring pass again.
// Every launch set, fresh or replayed, goes to the device through Batch::issue().
#include "engine.hpp"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>

namespace pml {
#define HIPCHK(expr)                                                                          \
    do { hipError_t e_ = (expr);                                                              \
         if (e_ != hipSuccess) return ctx->fail(-5, std::string(#expr) + ": " + hipGetErrorString(e_)); } while (0)
double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
// The environment switches of the launch path, read once per process, at its first launch.  PML_CHAIN, the A-B switch of
// register chaining (LaunchBuilder::build_descriptors): 2 = on (default), 1 = scoring passes only, 0 = off and the plain kernel only
// (no fused Newton); PML_NO_FUSE=1: the A-B arm of fused branch Newton; PML_SERIALIZE: diagnostic, a host sync after every launch
namespace {
struct Switches {
    const char *c = std::getenv("PML_CHAIN");
    int chain = c ? std::atoi(c) : 2;
    bool fuse = std::getenv("PML_NO_FUSE") == nullptr && chain != 0, serialize = std::getenv("PML_SERIALIZE") != nullptr;
};
const Switches &switches() { static const Switches s; return s; }
}  // namespace

// buffers of the launch path, grown on demand
// device -> host copy of the result buffers, enqueued behind the kernels that write them; the caller synchronises
int Batch::fetch_results(bool pooled) {
    HIPCHK(hipMemcpyAsync(h_scalars, d_scalars, sizeof(double) * scalars_doubles, hipMemcpyDeviceToHost, ctx->stream));
    if (pooled && results_used > 0 && d_chain)
        HIPCHK(hipMemcpyAsync(h_chain, d_chain, sizeof(double) * 4 * results_used, hipMemcpyDeviceToHost, ctx->stream));
    return 0;
}
int Batch::chain_sync() {
    if (int rc = flush_deferred()) return rc;
    if (int rc = fetch_results(true)) return rc;
    if (int rc = ctx->sync(ctx->stream)) return rc;
    HIPCHK(hipGetLastError());
    ctx->resolve_events();
    chain_off = 0;
    return 0;
}
int Batch::ensure_results(size_t nresults) {
    if (nresults > chain_cap) {
        if (h_chain) hipHostFree(h_chain);
        if (d_chain) hipFree(d_chain);
        h_chain = d_chain = nullptr; chain_cap = 0;
        const size_t cap = nresults * 3 / 2 + 64;
        HIPCHK(hipMalloc((void **)&d_chain, cap * 4 * sizeof(double)));
        HIPCHK(hipHostMalloc((void **)&h_chain, cap * 4 * sizeof(double), hipHostMallocDefault));
        chain_cap = cap;
    }
    results_used = nresults;
    return 0;
}
int Batch::ensure_tailpool(size_t bytes) {
    if (bytes <= tailpool_cap) return 0;
    if (d_tailpool) hipFree(d_tailpool);
    d_tailpool = nullptr; tailpool_cap = 0;
    if (hipMalloc((void **)&d_tailpool, bytes) != hipSuccess) { d_tailpool = nullptr; return ctx->fail(-4, "sumtable pool of " + std::to_string(bytes >> 20) + " MiB does not fit"); }
    tailpool_cap = bytes;
    return 0;
}
int Batch::chain_begin(size_t nresults) {
    if (int rc = ensure_results(nresults)) return rc;
    if (!d_lenpool) {
        size_t tot = 0; for (auto &G : genes) tot += (size_t)G.tree.nnodes() * 3;
        HIPCHK(hipMalloc((void **)&d_lenpool, tot * sizeof(double)));
        tot = 0; for (auto &G : genes) { G.d_len = d_lenpool + tot; tot += (size_t)G.tree.nnodes() * 3; }
    }
    for (auto &G : genes) G.len_pending.assign((size_t)G.tree.nnodes() * 3, 0);
    // descriptors of the whole pass stay in the staging ring until the final sync: ~4 KB per (gene, step) is what
    // run() reserves (it sizes for the worst case of 10 matrix requests per operation)
    if (int rc = ensure_stage(std::min<size_t>(nresults * 4096 + (1 << 20), (size_t)256 << 20))) return rc;
    chain = true; chain_off = 0; flush_quota = 1;
    return 0;
}
int Batch::ensure_stage(size_t bytes) {
    if (bytes <= h_cap) return 0;
    if (chain) { if (int rc = chain_sync()) return rc; }
    const size_t cap = std::max(bytes * 3 / 2, (size_t)1 << 20);
    if (h_stage) hipHostFree(h_stage);
    if (d_stage) hipFree(d_stage);
    h_stage = d_stage = nullptr; h_cap = d_cap = 0;
    HIPCHK(hipHostMalloc(&h_stage, cap));
    HIPCHK(hipMalloc(&d_stage, cap));
    h_cap = d_cap = cap;
    return 0;
}
int Batch::ensure_frags(size_t sets) {
    if (sets <= frag_cap) return 0;
    if (chain) { if (int rc = chain_sync()) return rc; }
    const size_t cap = std::max(sets * 5 / 4, (size_t)256);
    if (d_frags) hipFree(d_frags);
    d_frags = nullptr; frag_cap = 0;
    plan.valid = false;      // cached descriptors point into d_frags
    HIPCHK(hipMalloc((void **)&d_frags, cap * FRAG_STRIDE * sizeof(double)));
    frag_cap = cap;
    return 0;
}

// k_newton's exchange gave up
void Batch::newton_gave_up() {
    ++ctx->newton_giveups;
    if (std::getenv("PML_TRACE") && d_nctl) {
        NewtonCtl h;
        if (hipMemcpy(&h, d_nctl, sizeof h, hipMemcpyDeviceToHost) == hipSuccess)
            fprintf(stderr, "[pml] k_newton exchange gave up: slice %d of %d, evaluation %d, arrived mask %08x%08x, tickets taken in its partition %d, (left * 1024 + partition) %d; tickets %d %d done %d %d oticket %d %d %d %d %d %d %d %d odone %d\n",
                    h.dbg[1], h.dbg[2], h.dbg[3], (unsigned)h.dbg[5], (unsigned)h.dbg[4], (unsigned)h.dbg[6], h.dbg[7], h.ticket[0], h.ticket[1], h.done[0], h.done[1],
                    h.oticket[0], h.oticket[1], h.oticket[2], h.oticket[3], h.oticket[4], h.oticket[5], h.oticket[6], h.oticket[7], h.odone);
        hipMemset(&d_nctl->dbg[0], 0, sizeof(int));
    }
    safe_left = safe_hold; safe_hold = std::min(safe_hold * 2, 1024);
}
// the sticky abort word of the control block back to 0 (ordered on the batch's stream, then waited for)
int Batch::clear_abort() {
    if (!d_nctl) return 0;
    HIPCHK(hipMemsetAsync(&d_nctl->abort, 0, sizeof(int), ctx->stream));
    return ctx->sync(ctx->stream);
}
// k_pmat, k_oplist, k_reduce, then k_newton or its SEQ form, from the set's block at `ds` (device memory), on the batch's
// stream.  self_timed (a replayed plan): each launch records its own start and end (Ctx::tic_self), so that nothing but
// kernels sits in the queue; otherwise (a flushed step) each launch is bracketed by tic / toc and PML_SERIALIZE is honoured.
void Batch::issue(const LaunchSet &L, const char *ds, bool self_timed) {
    const hipStream_t st = ctx->stream;
    const ModelDev *md = d_gmodel ? nullptr : d_shared;      // per-gene models travel in the requests
    const bool serialize = !self_timed && switches().serialize;
    Ctx::Ev ev{0, nullptr, nullptr};
    auto begin = [&](int kind, double bytes, double flops) { if (self_timed) ev = ctx->tic_self(kind, bytes, flops); else ctx->tic(kind, bytes, flops); };
    auto end = [&] { if (!self_timed) ctx->toc(); if (serialize) hipStreamSynchronize(st); };
    if (L.nreq) {
        begin(K_PMAT, (double)L.nreq * PFRAG * 8, 0);
        launch_pmat(md, (const PmatReq *)(ds + L.o_req), d_frags, (int)L.nreq, st, d_gmodel != nullptr, ev.a, ev.b);
        end();
    }
    if (L.nruns) {
        begin(K_NEWVIEW, L.algo_bytes, L.algo_flops);
        launch_oplist((const NvOp *)(ds + L.o_ops), (const GeneRun *)(ds + L.o_runs), (int)L.nruns, L.max_mpad, L.any_pitch, L.any_chain, st, L.fused ? d_nctl : nullptr, ev.a, ev.b);
        end();
    }
    if (L.neval) {
        begin(K_REDUCE, 0, 0);
        launch_reduce((const ReduceReq *)(ds + L.o_red), (int)L.neval, st, ev.a, ev.b);
        end();
    }
    if (L.nt_reg + L.nt_stream > 0) {          // (no replayed plan has Newton tails: k_newton takes no events)
        begin(K_NEWTON, L.newton_bytes, 0);
        if (L.seq) { launch_newton_seq(md, (const NewtonReq *)(ds + L.o_newt), (const int *)(ds + L.o_tick), L.nt_reg, L.nt_stream, d_nctl, st); ++ctx->newton_seq_launches; }
        else launch_newton(md, (const NewtonReq *)(ds + L.o_newt), (const int *)(ds + L.o_tick), L.nt_reg, L.nt_stream, d_nctl, st);
        end();
    }
}
// one upload for all deferred steps (their descriptors are consecutive in the staging ring), then their launches in order
int Batch::flush_deferred() {
    if (deferred.empty()) return 0;
    // whatever happens below, the queue is empty afterwards: an error must not leave stale descriptors to be uploaded and
    // launched again by the next chain_sync() / run()
    struct Guard { Batch *b; ~Guard() { b->deferred.clear(); } } guard{this};
    const size_t lo = deferred.front().base, hi = deferred.back().base + deferred.back().set.bytes;
    HIPCHK(hipMemcpyAsync((char *)d_stage + lo, (char *)h_stage + lo, hi - lo, hipMemcpyHostToDevice, ctx->stream));
    if (switches().serialize) hipStreamSynchronize(ctx->stream);
    for (const Deferred &D : deferred) {
        issue(D.set, (const char *)d_stage + D.base, false);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return ctx->fail(-5, std::string("kernel launch: ") + hipGetErrorString(e));
    }
    flush_quota = std::min<size_t>(flush_quota * 2, 8);
    return 0;
}

// run: one upload, pmat, newview levels, tails, one sync
namespace {
// one resolved side of an operation: pointers, kind, scaling counts
// bytes / flops: SURVEY 8d's per-operation figures (newview inner-inner 1920 B / 6480 flop, tip-inner 1281 B / 3280 flop,
// tip-tip 642 B / 80 flop, evaluate 1280 B / 3360 flop per pattern).  `inner`: the side counts as an inner child of the
// operation; `flops`: work 8d assigns to producing a side that is never materialised (virtual cherry = one tip-tip newview,
// virtual pitchfork = that + one tip-inner newview)
struct Resolved { OpSide s; int kind; const int *scl; double bytes; double flops = 0; bool inner = true; };
// Builds the staging block of one run() call and sees it through.  run() calls the stages in order: size_block, reserve,
// build_descriptors, build_tickets, submit, complete (unless chained), mark_valid, keep_plan (when one is being recorded).
struct LaunchBuilder {
    using Tail = Batch::Tail;
    Batch &b; Ctx *const ctx; Batch::LaunchScratch &sc;
    std::vector<PendingOp> &ops; const std::vector<Tail> &tails; const size_t nops, ntail;
    size_t nnewton = 0, nreq_max = 0, nkeys = 0, base = 0;
    LaunchSet L;                                   // offsets and bytes from size_block(); counts, flags and figures as the build goes
    // host and device address of the staging block, the six arrays in the host block
    char *hs = nullptr, *ds = nullptr;
    PmatReq *hreq = nullptr; NvOp *hops = nullptr; GeneRun *hruns = nullptr; ReduceReq *hred = nullptr; NewtonReq *hnewt = nullptr; int *htick = nullptr;
    size_t ireq = 0, nout = 0, ie = 0, in = 0, iop = 0;      // requests, descriptors, reductions, Newton requests written; next operation
    bool req_overflow = false, fuse_ok = false, chain_reads = false, chain_nostore = false; unsigned tag_base = 0;
    // the run (gene, part) being built
    size_t g = 0, key = 0, ti = 0;                 // gene, index into tails_of, tails of the run emitted so far
    int mp = 0, emitted = 0;                       // the gene's mpad, newviews of the run emitted so far
    long last_nv = -1, last_nv_op = -1;            // hops / ops index of the gene's last newview

    bool chained_from(const Side &sd, int kind) const {
        return chain_reads && last_nv >= 0 && kind == SK_CLV && sd.kind == ops[last_nv_op].out_kind && sd.id == ops[last_nv_op].out_id;
    }
    void consume_last() {                          // the last newview's result is taken from the registers by the operation being built
        L.any_chain = true;
        if (chain_nostore || ops[last_nv_op].transient) { hops[last_nv].flags |= OPF_NO_STORE; ops[last_nv_op].unstored = true; }
    }
    const double *result_of(const Tail &t) const { return t.result_host ? t.result_host : (t.result_dev ? (const double *)nullptr : b.res(t.gene, t.slot)); }
    // stage 1: the bound on transition-matrix requests, the runs of the launch, the layout of the staging block
    void size_block() {
        auto &genes = b.genes;
        for (auto &t : tails) { if (t.mode == MODE_EVALUATE) L.neval++; else if (t.mode != MODE_EVALUATE_CAT) nnewton++; }
        // <= 5 requests per side (pitchfork: 3 tables + 2 fragment sets) -- but requests across the same tree branch are
        // shared within the launch (add_req), so a gene never needs more than 5 per taxon plus those of lengths that
        // belong to no branch of the tree (SPR path / insertion operations)
        std::vector<char> seen(genes.size(), 0);
        size_t keyed = 0, loose = 0;
        for (auto &o : ops) { if (!seen[o.gene]) { seen[o.gene] = 1; keyed += 5 * (size_t)genes[o.gene].aln.ntax; }
                              if (o.out_kind != SIDE_MSG) loose += (o.bv[0] < 0) + (o.bv[1] < 0); }      // one fragment set per child whose length is no tree branch
        for (auto &t : tails) { if (!seen[t.gene]) { seen[t.gene] = 1; keyed += 5 * (size_t)genes[t.gene].aln.ntax; }
                                if (t.mode >= MODE_EVALUATE && t.bv < 0) loose += 1; }
        nreq_max = std::min(10 * nops + 9 * ntail, keyed + loose);
        // runs of the launch: one per (gene, part) -- parts of a gene are independent of each other (PendingOp::part)
        const size_t ngenes = genes.size();
        std::vector<int> &nparts = sc.run_nparts; nparts.assign(ngenes, 1);
        for (auto &o : ops) nparts[o.gene] = std::max(nparts[o.gene], o.part + 1);
        for (auto &t : tails) nparts[t.gene] = std::max(nparts[t.gene], t.part + 1);
        std::vector<size_t> &koff = sc.run_koff; koff.assign(ngenes + 1, 0);
        for (size_t g_ = 0; g_ < ngenes; ++g_) koff[g_ + 1] = koff[g_] + (size_t)nparts[g_];
        nkeys = koff[ngenes];
        L.o_ops = align_up(L.o_req + nreq_max * sizeof(PmatReq), 256);
        L.o_runs = align_up(L.o_ops + (nops + ntail) * sizeof(NvOp), 256);
        L.o_red = align_up(L.o_runs + nkeys * sizeof(GeneRun), 256);
        L.o_newt = align_up(L.o_red + L.neval * sizeof(ReduceReq), 256);
        size_t ntick_max = 0;                          // k_newton tickets: one per (request, slice)
        for (auto &t : tails) if (t.mode == MODE_SUMTABLE) ntick_max += (size_t)newton_split(genes[t.gene].aln.mpad);
        L.o_tick = align_up(L.o_newt + nnewton * sizeof(NewtonReq), 256);
        L.bytes = align_up(L.o_tick + ntick_max * sizeof(int), 256);
    }
    // stage 2: fragment sets, Newton sync and control blocks, and this launch set's place in the staging buffer (ring)
    int reserve() {
        if (int rc = b.ensure_frags(std::max(nreq_max, (size_t)1))) return rc;
        if (nnewton > b.nsync_cap) {
            if (b.chain) { if (int rc = b.chain_sync()) return rc; }
            if (b.d_nsync) hipFree(b.d_nsync);
            b.d_nsync = nullptr; b.nsync_cap = 0;
            const size_t cap = std::max(nnewton * 2, (size_t)256);
            HIPCHK(hipMalloc((void **)&b.d_nsync, cap * NEWTON_SYNC_DOUBLES * sizeof(double)));
            // granule tags are (launch number << 10) + evaluation: a fresh block must not hold a matching tag by accident
            HIPCHK(hipMemsetAsync(b.d_nsync, 0, cap * NEWTON_SYNC_DOUBLES * sizeof(double), ctx->stream));
            if (int rc = ctx->sync(ctx->stream)) return rc;
            b.nsync_cap = cap;
        }
        if (nnewton && !b.d_nctl) {
            HIPCHK(hipMalloc((void **)&b.d_nctl, sizeof(NewtonCtl)));
            // ON THE BATCH'S STREAM and waited for: a null-stream hipMemset returns before it has run and is not ordered against the
            // non-blocking streams the kernels use -- landing inside the first k_newton it would re-issue tickets and leave the
            // counters un-armed for the next launch (seen as time-outs and a memory fault when several batches shared the device)
            HIPCHK(hipMemsetAsync(b.d_nctl, 0, sizeof(NewtonCtl), ctx->stream));
            if (int rc = ctx->sync(ctx->stream)) return rc;
        }
        if (b.chain && b.chain_off + L.bytes > b.h_cap) { if (int rc = b.chain_sync()) return rc; }     // ring full: drain, start over
        if (int rc = b.ensure_stage(L.bytes)) return rc;
        base = b.chain ? b.chain_off : 0;
        if (b.chain) b.chain_off += L.bytes;
        hs = (char *)b.h_stage + base; ds = (char *)b.d_stage + base;
        hreq = (PmatReq *)(hs + L.o_req); hops = (NvOp *)(hs + L.o_ops); hruns = (GeneRun *)(hs + L.o_runs);
        hred = (ReduceReq *)(hs + L.o_red); hnewt = (NewtonReq *)(hs + L.o_newt); htick = (int *)(hs + L.o_tick);
        return 0;
    }
    // The request tables of this launch.  One transition-matrix request per (gene, kind, tree branch) and launch; never while
    // a plan is being recorded (a replay refreshes each request from ITS branch).
    // keyed requests live in a flat table stamped with the launch number (no hashing, nothing to clear): one entry per
    // (gene, kind, directed branch slot); the undirected branch is the smaller of its two slots
    void prepare_requests() {
        auto &genes = b.genes;
        sc.last_src.clear();
        bool req_ok = sc.req_off.size() == genes.size() + 1;
        for (size_t g_ = 0; req_ok && g_ < genes.size(); ++g_) req_ok = sc.req_off[g_ + 1] - sc.req_off[g_] == (size_t)9 * genes[g_].tree.nnodes();
        if (!req_ok) {
            sc.req_off.assign(genes.size() + 1, 0);
            for (size_t g_ = 0; g_ < genes.size(); ++g_) sc.req_off[g_ + 1] = sc.req_off[g_] + (size_t)3 * 3 * genes[g_].tree.nnodes();
            sc.req_stamp.assign(sc.req_off.back(), 0); sc.req_ptr.assign(sc.req_off.back(), nullptr); sc.req_launch = 0;
            sc.val_bucket.assign(genes.size() * 3, {}); sc.val_stamp.assign(genes.size() * 3, 0);
        }
        if (++sc.req_launch == 0) {                    // the 32-bit launch number wrapped: no stale stamp may match it
            std::fill(sc.req_stamp.begin(), sc.req_stamp.end(), 0u); std::fill(sc.val_stamp.begin(), sc.val_stamp.end(), 0u); sc.req_launch = 1;
        }
    }
    // one transition-matrix request (fragment set or tip table) for branch (v, slot q) of the current gene
    // requests whose length belongs to no branch of the tree (v < 0; SPR: joined / halved branches) are shared by VALUE: the
    // same (gene, kind, length) gives the same matrices: one list of (length bits, matrices) per (gene, kind).
    const double *add_req(double t, int kind, int v, int q) {
        Gene &G = b.genes[g];
        uint64_t tbits = 0; size_t rkey = 0;
        std::vector<std::pair<uint64_t, const double *>> *bucket = nullptr;
        if (!b.record_plan) {
            if (v >= 0) {
                const Tree &T = G.tree;
                const int w = T.nbr[v][q], a = v * 3 + q, c = w * 3 + T.slot(w, v);
                rkey = sc.req_off[g] + (size_t)kind * 3 * T.nnodes() + (size_t)std::min(a, c);
                if (sc.req_stamp[rkey] == sc.req_launch) return sc.req_ptr[rkey];
            } else {
                std::memcpy(&tbits, &t, 8);
                const size_t bi = g * 3 + (size_t)kind;                              // exact (gene, kind); a few hundred lengths at most
                if (sc.val_stamp[bi] != sc.req_launch) { sc.val_bucket[bi].clear(); sc.val_stamp[bi] = sc.req_launch; }
                bucket = &sc.val_bucket[bi];
                for (auto &e : *bucket) if (e.first == tbits) return e.second;
            }
        }
        if (ireq >= nreq_max) { req_overflow = true; return b.d_frags; }      // reported after the build (build_descriptors)
        PmatReq &r = hreq[ireq];
        r.t = t; std::memcpy(r.rates, G.rates, sizeof r.rates); r.kind = kind; r.pad = 0;
        r.tp = (b.chain && v >= 0 && G.len_pending[(size_t)v * 3 + q]) ? G.d_len + (size_t)v * 3 + q : nullptr;
        r.md = b.d_gmodel ? b.d_gmodel + g : nullptr;
        sc.last_src.push_back({(int)g, v, q, kind});
        const double *out = b.d_frags + (ireq++) * FRAG_STRIDE;
        if (!b.record_plan) { if (v >= 0) { sc.req_stamp[rkey] = sc.req_launch; sc.req_ptr[rkey] = out; } else bucket->push_back({tbits, out}); }
        return out;
    }
    // resolves one side of an operation of the current gene (Resolved); cherry and pitchfork sides request their tip tables
    // (and the fragments of the branch to the cherry) here
    int resolve(const Side &sd, Resolved &R) {
        Gene &G = b.genes[g];
        const int nt = G.aln.ntax;
        R.s = OpSide{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}; R.scl = nullptr;
        R.flops = 0; R.inner = true;
        if (sd.kind == SIDE_TIP) { R.kind = SK_TIP; R.s.p0 = G.d_codes + (size_t)sd.id * mp; R.bytes = 1; R.inner = false; return 0; }
        if (sd.kind == SIDE_CHERRY) {
            const int v = nt + sd.id / 3, k = sd.id % 3;
            int tips[2], qs[2], ci = 0;
            for (int q = 0; q < 3; ++q) if (q != k) { tips[ci] = G.tree.nbr[v][q]; qs[ci] = q; ++ci; }
            R.kind = SK_CHERRY;
            R.s.p0 = G.d_codes + (size_t)tips[0] * mp; R.s.p1 = G.d_codes + (size_t)tips[1] * mp;
            R.s.t0 = add_req(G.tree.len[v][qs[0]], PM_TIPTABLE, v, qs[0]);
            R.s.t1 = add_req(G.tree.len[v][qs[1]], PM_TIPTABLE, v, qs[1]);
            R.bytes = 640 + 642;       // SURVEY 8d accounting: the tip-tip newview (642 B) + reading its CLV (640 B)
            R.flops = 80;
            return 0;
        }
        if (sd.kind == SIDE_PITCH) {
            // X over (cherry C = tips a,b ; tip c): tables of a,b,c + the fragments of branch X-C
            const int X = nt + sd.id / 3, k = sd.id % 3;
            int qc = -1, qC = -1;
            for (int q = 0; q < 3; ++q) if (q != k) { if (G.tree.nbr[X][q] < nt) qc = q; else qC = q; }
            const int C = G.tree.nbr[X][qC], kC = G.tree.slot(C, X);
            int tips[2], qs[2], ci = 0;
            for (int q = 0; q < 3; ++q) if (q != kC) { tips[ci] = G.tree.nbr[C][q]; qs[ci] = q; ++ci; }
            R.kind = SK_PITCH;
            R.s.p0 = G.d_codes + (size_t)tips[0] * mp; R.s.p1 = G.d_codes + (size_t)tips[1] * mp;
            R.s.p2 = G.d_codes + (size_t)G.tree.nbr[X][qc] * mp;
            R.s.t0 = add_req(G.tree.len[C][qs[0]], PM_TIPTABLE, C, qs[0]);
            R.s.t1 = add_req(G.tree.len[C][qs[1]], PM_TIPTABLE, C, qs[1]);
            R.s.t2 = add_req(G.tree.len[X][qc], PM_TIPTABLE, X, qc);
            R.s.f = add_req(G.tree.len[X][qC], PM_FRAGS, X, qC);
            L.any_pitch = true;
            R.bytes = 640 + (640 + 642) + 1 + 640;   // read X + X's newview (cherry child, tip child, write)
            R.flops = 80 + 3280;
            return 0;
        }
        const int slot = sd.kind == SIDE_MSG ? G.slot_of[sd.id] : G.slot_cap + sd.id;
        if (slot < 0) return -1;
        R.kind = SK_CLV; R.s.p0 = G.d_clv + (size_t)slot * clv_doubles(mp); R.scl = G.d_scl + (size_t)slot * mp; R.bytes = 640;
        return 0;
    }
    // the descriptor of one tail of the current run: an evaluation (with its reduction request) or a sumtable operation with
    // its Newton request, fused into the operation where that is possible
    int emit_tail(const Tail &t) {
        Gene &G = b.genes[g];
        NvOp &d = hops[nout++];
        std::memset(&d, 0, sizeof d);
        Resolved Lt, Rt;
        if (resolve(t.a, Lt) || resolve(t.b, Rt)) return ctx->fail(-5, "internal: tail message has no slot");
        d.l = Lt.s; d.r = Rt.s; d.l_scl = Lt.scl; d.r_scl = Rt.scl;
        d.flags = Lt.kind | (Rt.kind << 2); d.mpad = mp; d.mode = t.mode;
        if (chained_from(t.a, Lt.kind)) { d.flags |= OPF_CHAIN_L; consume_last(); }
        else if (t.mode >= MODE_EVALUATE && chained_from(t.b, Rt.kind)) { d.flags |= OPF_CHAIN_R; consume_last(); }
        double *result = t.result_dev ? t.result_dev : b.d_scalars + 8 * (g * MAXTAIL + t.slot);
        if (t.mode == MODE_EVALUATE_CAT) {
            if (!t.patlnl_dev || !t.scl_dev) return ctx->fail(-1, "internal: table slice missing");
            d.pl = d.pr = add_req(t.t0, PM_FRAGS_PI, t.bv, t.bq);
            d.out = t.patlnl_dev; d.out_scl = t.scl_dev;
            L.algo_bytes += (double)G.aln.npat * (Lt.bytes + Rt.bytes + 36);
            L.algo_flops += (double)G.aln.npat * (3360 + Lt.flops + Rt.flops);
        } else if (t.mode == MODE_EVALUATE) {
            d.pl = d.pr = add_req(t.t0, PM_FRAGS_PI, t.bv, t.bq);
            double *pl = t.patlnl_dev ? t.patlnl_dev : G.d_patlnl[t.slot];      // pooled when a gene has more than MAXTAIL tails
            d.out = pl; d.out_scl = nullptr;
            ReduceReq &rr = hred[ie++];
            rr.patlnl = pl; rr.weight = G.d_weight; rr.out = result; rr.mpad = mp; rr.pad = 0;
            L.algo_bytes += (double)G.aln.npat * (Lt.bytes + Rt.bytes + 8);
            L.algo_flops += (double)G.aln.npat * (3360 + Lt.flops + Rt.flops);
        } else {
            d.pl = b.eig_of((int)g); d.pr = d.pl + PFRAG;
            double *stab = t.sumtab_dev ? t.sumtab_dev : G.d_sumtab[t.slot];
            int *sscl = t.sumtab_dev ? reinterpret_cast<int *>(t.sumtab_dev + clv_doubles(mp)) : G.d_sumscl[t.slot];
            d.out = stab; d.out_scl = sscl;
            NewtonReq &nr = hnewt[in];
            nr.md = b.model_of((int)g); nr.tag_base = tag_base; nr.pad0 = 0;
            // (any number of tails per gene, anywhere in its list: every request has its own exchange block, the gene's workgroups
            // walk the list in step.  An NNI round -- three tails per internal edge -- then neither writes nor re-reads its pooled
            // sumtables, 640 B per pattern and tail)
            if (fuse_ok && !t.patlnl_dev && newton_reg_form(mp)) {
                d.flags |= OPF_FUSED_NEWTON; d.aux = (const NewtonReq *)(ds + L.o_newt) + in;
                sc.fused_req[in] = 1; L.fused = true; L.any_chain = true;
            }
            last_nv = -1; last_nv_op = -1;              // a sumtable operation leaves ITS tile in the wave's registers (kernels.hip chunk_op): the chain ends here
            sc.tail_req[&t - tails.data()] = (int)in;
            nr.ticket0 = 0; nr.pad = 0;
            nr.sumtab = stab; nr.weight = G.d_weight; nr.scl = sscl;
            std::memcpy(nr.rates, G.rates, sizeof nr.rates);
            nr.t0 = t.t0; nr.tol = b.newton_tol; nr.out = result; nr.mpad = mp; nr.max_iter = t.max_iter;
            nr.t_dev0 = t.t_dev0; nr.t_dev1 = t.t_dev1; nr.patlnl = t.patlnl_dev;
            nr.sync = b.d_nsync + (size_t)in * NEWTON_SYNC_DOUBLES;
            L.algo_bytes += (double)G.aln.npat * (Lt.bytes + Rt.bytes + 640);
            L.algo_flops += (double)G.aln.npat * (6480 + Lt.flops + Rt.flops);      // the newview contraction with the eigen-basis matrices
            in++;
        }
        return 0;
    }
    // the tails of the current run that are due: all of them, or those placed after no more newviews than have been emitted
    int flush_tails(bool all) {
        const std::vector<int> &mine = sc.run_tails_of[key];
        while (ti < mine.size()) {
            const Tail &t = tails[mine[ti]];
            if (!all && (t.after < 0 || t.after > emitted)) break;
            if (int rc = emit_tail(t)) return rc;
            ++ti;
        }
        return 0;
    }
    // the descriptor of newview operation ops[iop] of the current run
    int emit_op(PendingOp &o) {
        Gene &G = b.genes[g];
        const int s = o.out_kind == SIDE_MSG ? b.slot_for(G, o.out_id) : G.slot_cap + o.out_id;
        if (s < 0) return ctx->fail(-4, "CLV slots exhausted (score-only batch used for a multi-root request)");
        NvOp &d = hops[nout++];
        std::memset(&d, 0, sizeof d);
        d.mode = MODE_NEWVIEW;
        d.out = G.d_clv + (size_t)s * clv_doubles(mp);
        d.out_scl = G.d_scl + (size_t)s * mp;
        Resolved S[2];
        if (resolve(o.child[0], S[0]) || resolve(o.child[1], S[1])) return ctx->fail(-5, "internal: child message has no slot");
        d.mpad = mp;
        const double *pm[2];
        for (int c = 0; c < 2; ++c) {
            // where this child's branch length lives (plan replay): output message (v, k), child c
            int bv = o.bv[c], bq = o.bq[c];
            if (o.out_kind == SIDE_MSG) {
                bv = G.aln.ntax + o.out_id / 3; const int k = o.out_id % 3;
                int seen = 0;
                for (bq = 0; bq < 3; ++bq) if (bq != k) { if (seen == c) break; ++seen; }
            }
            pm[c] = add_req(o.t[c], PM_FRAGS, bv, bq);
        }
        // the child that is the gene's previous result goes LEFT (the two factors of a newview commute bit for bit)
        // (the PendingOp itself keeps its order: t[], bv[], bq[] belong to its children by position, and a launch set that has to
        // be issued again -- run()'s retry in safe mode -- must find it unchanged)
        Side ch[2] = {o.child[0], o.child[1]};
        if (chained_from(ch[1], S[1].kind)) { std::swap(S[0], S[1]); std::swap(pm[0], pm[1]); std::swap(ch[0], ch[1]); }
        d.flags = S[0].kind | (S[1].kind << 2);
        if (chained_from(ch[0], S[0].kind)) { d.flags |= OPF_CHAIN_L; consume_last(); }
        d.l = S[0].s; d.r = S[1].s; d.l_scl = S[0].scl; d.r_scl = S[1].scl; d.pl = pm[0]; d.pr = pm[1];
        L.algo_bytes += (double)G.aln.npat * (S[0].bytes + S[1].bytes + 640);
        L.algo_flops += (double)G.aln.npat * ((S[0].inner && S[1].inner ? 6480 : (S[0].inner || S[1].inner ? 3280 : 80)) + S[0].flops + S[1].flops);
        last_nv = (long)nout - 1; last_nv_op = (long)iop;
        ++emitted;
        return 0;
    }
    // one run of the launch: the operations of (gene g, part) in order, each tail behind the newview it was placed after
    int build_run(int part) {
        key = sc.run_koff[g] + (size_t)part;
        const bool has_ops = iop < nops && ops[iop].gene == (int)g && ops[iop].part == part;
        if (!has_ops && sc.run_tails_of[key].empty()) return 0;
        mp = b.genes[g].aln.mpad;
        GeneRun &run = hruns[L.nruns++];
        run.op_begin = (int)nout;
        L.max_mpad = std::max(L.max_mpad, mp);
        last_nv = -1; last_nv_op = -1; ti = 0; emitted = 0;
        if (int rc = flush_tails(false)) return rc;
        for (; iop < nops && ops[iop].gene == (int)g && ops[iop].part == part; ++iop) {
            if (int rc = emit_op(ops[iop])) return rc;
            if (int rc = flush_tails(false)) return rc;
        }
        if (int rc = flush_tails(true)) return rc;
        run.op_end = (int)nout;
        // Cache policy of the CLV stores, per gene.  Measured on one box, rotated order (profiles/r02_ab_nontemporal.txt): with
        // NON-TEMPORAL stores the C3 scoring launch (8 tiles per gene) takes 0.89 ms instead of 0.98 -- written CLVs no longer
        // push the transition-matrix fragments and tip tables out of L2 / Infinity Cache, which 8 workgroups per gene re-fetch
        // for every operation -- while the C4 shard (40 tiles per gene: 40 workgroups share each fragment set, and a parent
        // often finds its child's CLV still in the Infinity Cache) takes 10.15 ms instead of 9.18.  Hence by gene size.
        if (mp <= 16 * TILE_PAT)
            for (int i = run.op_begin; i < run.op_end; ++i) if (hops[i].mode == MODE_NEWVIEW) hops[i].flags |= OPF_NT_STORE;
        return 0;
    }
    // stage 3: requests, operations, reductions and Newton requests of every run into the staging block
    int build_descriptors() {
        if (nnewton) ++b.newton_launch_seq;
        tag_base = (b.newton_launch_seq & 0x3FFFFFu) << 10;
        // fused branch Newton (kernels.h OPF_FUSED_NEWTON): a gene's only Newton tail, sitting behind all of its operations, is
        // iterated inside k_oplist<11> on the register-resident sumtable; PML_NO_FUSE=1 is the A-B arm, safe mode (after an exchange
        // gave up) runs unfused through the no-exchange k_newton form
        // (genes of more than 32 tiles: kernels.hip launch_oplist -- one launch with one ticket partition over the device.  Fusing
        // them only when the whole launch is resident at once, cut into several resident launches, paid the Newton latency once per
        // launch and measured slower than un-fused on a C4 shard)
        fuse_ok = switches().fuse && !b.newton_safe_mode();
        // Register chaining (kernels.h OPF_CHAIN_*): the gene's last newview result is still in the registers of the wave
        // that owns the patterns.  Every launch takes a child that the directly following operation of the gene consumes
        // from there instead of reading it back; whole-tree scoring passes (record_plan), whose results nobody reads
        // again, do not even write such a child (it stays invalid in memory and is recomputed if a later request wants it).
        // PML_CHAIN (A-B switch): 2 = that (default), 1 = scoring passes only, 0 = off.  Measured on one box, rotated order
        // (profiles/r02_ab_register_chaining.txt): C3 scoring launch 0.89 -> 0.72 ms, C4 shard 3.40 -> 2.92 ms, C3 search
        // 153 -> 161 gene-trees/s.
        const int chain_env = switches().chain;
        chain_reads = chain_env == 2 || (chain_env == 1 && b.record_plan); chain_nostore = chain_env >= 1 && b.record_plan && !b.record_stored;
        sc.fused_req.assign(nnewton, 0);
        sc.tail_req.assign(ntail, -1);                 // tail -> index of its NewtonReq (failure handling in complete())
        prepare_requests();
        // tails by gene, in submission order (<= MAXTAIL per gene per run)
        std::vector<std::vector<int>> &tails_of = sc.run_tails_of;          // kept between launches: no allocations per launch
        if (tails_of.size() < nkeys) tails_of.resize(nkeys);
        for (auto &v : tails_of) v.clear();
        for (size_t i = 0; i < ntail; ++i) {
            if (tails[i].slot < 0 || tails[i].slot >= MAXTAIL) return ctx->fail(-1, "internal: bad tail slot");
            tails_of[sc.run_koff[tails[i].gene] + (size_t)tails[i].part].push_back((int)i);
        }
        for (g = 0; g < b.genes.size(); ++g)
            for (int part = 0; part < sc.run_nparts[g]; ++part) if (int rc = build_run(part)) return rc;
        L.nreq = ireq;
        if (req_overflow) return ctx->fail(-5, "internal: transition-matrix request bound exceeded");
        return 0;
    }
    // stage 4: k_newton's ticket table: (request, slice) in request order, register-form requests first, then the streaming-form
    // ones (genes of more than 8192 patterns); in safe mode (SEQ form) one entry per request instead.  Fused requests get none.
    void build_tickets() {
        L.seq = nnewton > 0 && b.newton_safe_mode();
        int cur = 0;
        for (int pass = 0; pass < 2; ++pass) {
            for (size_t i = 0; i < nnewton; ++i) {
                if (sc.fused_req[i] || newton_reg_form(hnewt[i].mpad) != (pass == 0)) continue;
                const int S = L.seq ? 1 : newton_split(hnewt[i].mpad);
                hnewt[i].ticket0 = cur - (pass == 0 ? 0 : L.nt_reg);            // relative to its kernel's table
                for (int k = 0; k < S; ++k) htick[cur++] = (int)i;
            }
            if (pass == 0) L.nt_reg = cur; else L.nt_stream = cur - L.nt_reg;
        }
        if (nnewton && b.safe_left > 0 && !b.safe_now) --b.safe_left;
        for (size_t i = 0; i < ntail; ++i)
            if (tails[i].mode == MODE_SUMTABLE && !sc.fused_req[sc.tail_req[i]]) L.newton_bytes += (double)b.genes[tails[i].gene].aln.npat * 640;
    }
    // stage 5: upload and launch -- at once, or inside a chained pass DEFERRED and issued in groups (1, 2, 4, 8, 8, ... steps):
    // a host-to-device copy between two kernels of one stream costs a ~20 us bubble on the compute queue (measured:
    // 2866 newton -> pmat gaps of 21 us in a C3 search, profiles/r02b), one copy per group leaves a handful per pass.
    // The host keeps building the next group while the device works on the last one.
    int submit() { b.deferred.push_back({L, base}); return !b.chain || b.deferred.size() >= b.flush_quota ? b.flush_deferred() : 0; }
    // stage 6 (not in a chained pass): wait for the results; Newton requests whose exchange gave up are issued again -- un-fused
    // ones here through the SEQ form, a launch set with a fused one as a whole (retry: run() runs the same ops / tails again)
    int complete(double t_begin, double t_launched, bool &retry) {
        bool pooled = false;
        for (auto &t : tails) pooled = pooled || t.result_host != nullptr;
        if (int rc = b.fetch_results(pooled)) return rc;
        if (int rc = ctx->sync(ctx->stream)) return rc;
        HIPCHK(hipGetLastError());
        const double t_done = now_ms();
        ctx->stats[K_HOST_WAIT].launches++; ctx->stats[K_HOST_WAIT].ms += t_done - t_launched;
        b.host_phase_ms[Batch::HP_RUN_SYNCED] += t_launched - t_begin;           // descriptor build of a launch the device waited for
        ctx->resolve_events();
        // A Newton request whose cross-workgroup exchange gave up reports lnL = NaN (k_newton).  Its sumtable is still in
        // place: the affected requests are re-issued through the no-exchange SEQ form (one workgroup walks the slices; the
        // bits of the split form), here, before anybody consumes a result.
        std::vector<int> bad;
        for (size_t i = 0; i < ntail; ++i) {
            const Tail &t = tails[i];
            if (t.mode != MODE_SUMTABLE) continue;
            const double *h = result_of(t);
            if (h && !std::isfinite(h[1])) bad.push_back(sc.tail_req[i]);
        }
        bool bad_fused = false;
        for (int i : bad) bad_fused = bad_fused || sc.fused_req[i];
        if (bad_fused && !b.in_retry) {
            // a fused request has no stored sumtable to iterate on: the whole launch set runs again, unfused, through the
            // no-exchange form (newton_gave_up() puts the batch in safe mode); CLV results are recomputed to the same bits
            b.newton_gave_up(); ctx->newton_reissued += (long long)bad.size();
            if (int rc = b.clear_abort()) return rc;
            for (auto &o : ops) { o.unstored = false; if (o.out_kind == SIDE_MSG) b.genes[o.gene].pend_level[o.out_id] = -1; }
            retry = true;
            return 0;
        }
        if (!bad.empty() && !L.seq && !bad_fused) {
            b.newton_gave_up(); ctx->newton_reissued += (long long)bad.size();
            int nr = 0, ns = 0;
            for (int pass = 0; pass < 2; ++pass) for (int i : bad) if (newton_reg_form(hnewt[i].mpad) == (pass == 0)) { htick[nr + ns] = i; ++(pass == 0 ? nr : ns); }
            if (int rc = b.clear_abort()) return rc;
            HIPCHK(hipMemcpyAsync(ds + L.o_tick, hs + L.o_tick, bad.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
            launch_newton_seq(nullptr, (const NewtonReq *)(ds + L.o_newt), (const int *)(ds + L.o_tick), nr, ns, b.d_nctl, ctx->stream);
            ++ctx->newton_seq_launches;
            if (int rc = b.fetch_results(pooled)) return rc;
            if (int rc = ctx->sync(ctx->stream)) return rc;
            HIPCHK(hipGetLastError());
        }
        for (auto &t : tails) {
            if (t.mode == MODE_EVALUATE_CAT) continue;
            const double *h = result_of(t);
#ifndef ABL_KEEP_GOING      // timing-only ablation builds (tools/ab_w1_ablation.sh) compute garbage on purpose
            if (h && !std::isfinite(t.mode == MODE_EVALUATE ? h[0] : h[1]))
                return ctx->fail(-5, t.mode == MODE_EVALUATE ? "device returned a non-finite likelihood" : "k_newton: non-finite branch likelihood (also from the no-exchange form)");
#endif
        }
        return 0;
    }
    // stage 7: the messages this launch computed are valid, unless their result stayed in registers
    void mark_valid() { for (auto &o : ops) if (o.out_kind == SIDE_MSG) { Gene &G = b.genes[o.gene]; G.valid[o.out_id] = o.unstored ? 0 : 1; G.pend_level[o.out_id] = -1; } }
    // stage 8: keep the descriptors of this full-traversal score (a byte copy of the staging block) for replay_plan()
    int keep_plan() {
        auto &genes = b.genes;
        b.record_plan = false;
        Batch::Plan &P = b.plan;
        if (P.cap < L.bytes) {
            if (P.h) hipHostFree(P.h);
            if (P.d) hipFree(P.d);
            P.h = P.d = nullptr; P.cap = 0;
            HIPCHK(hipHostMalloc(&P.h, L.bytes)); HIPCHK(hipMalloc(&P.d, L.bytes)); P.cap = L.bytes;
        }
        std::memcpy(P.h, hs, L.bytes);
        // ON THE BATCH'S STREAM: a device-to-device hipMemcpy returns before the copy ran and the null stream is not
        // ordered against the (non-blocking) stream a replay uploads its refreshed requests on -- the late copy then
        // put the recorded rates back under the first replay (DESIGN r02-g: the cause of the rare different optimum)
        HIPCHK(hipMemcpyAsync(P.d, ds, L.bytes, hipMemcpyDeviceToDevice, ctx->stream));
        // a replay returns one lnL per gene: its reductions write into d_plan_lnl (gene order) instead of the result slots
        ReduceReq *pred = (ReduceReq *)((char *)P.h + L.o_red);
        P.per_gene = L.neval == genes.size();
        for (size_t g_ = 0; P.per_gene && g_ < L.neval; ++g_) P.per_gene = pred[g_].out == b.d_scalars + 8 * (g_ * MAXTAIL);      // request g is gene g's
        if (P.per_gene) {
            for (size_t g_ = 0; g_ < L.neval; ++g_) pred[g_].out = b.d_plan_lnl + g_;
            HIPCHK(hipMemcpyAsync((char *)P.d + L.o_red, pred, L.neval * sizeof(ReduceReq), hipMemcpyHostToDevice, ctx->stream));
        }
        P.len_seen.assign(genes.size(), 0);
        P.check_len = std::getenv("PML_CHECK_LEN_STAMP") != nullptr;
        P.len_copy.assign(P.check_len ? genes.size() : 0, {});
        P.set = L; P.stored = b.record_stored;
        P.rates_seen.resize(genes.size()); for (size_t g_ = 0; g_ < genes.size(); ++g_) P.rates_seen[g_] = genes[g_].rates_epoch;
        P.src = sc.last_src; P.outs.clear();
        for (auto &o : ops) if (o.out_kind == SIDE_MSG && !o.unstored) P.outs.push_back({o.gene, o.out_id});
        P.epoch = b.topo_epoch; P.valid = true;
        return 0;
    }
};
}  // namespace
int Batch::run(std::vector<PendingOp> &ops, const std::vector<Tail> &tails) {
    const double t_begin = now_ms();
    HIPCHK(hipSetDevice(ctx->device));
    // group by gene, keeping each gene's dependency order (children are emitted before parents)
    std::stable_sort(ops.begin(), ops.end(), [](const PendingOp &a, const PendingOp &b) { return a.gene != b.gene ? a.gene < b.gene : a.part < b.part; });
    LaunchBuilder B{*this, ctx, scratch, ops, tails, ops.size(), tails.size()};
    B.size_block();
    if (int rc = B.reserve()) return rc;
    if (int rc = B.build_descriptors()) return rc;
    B.build_tickets();
    if (int rc = B.submit()) return rc;
    const double t_launched = now_ms();
    ctx->stats[K_HOST_BUILD].launches++; ctx->stats[K_HOST_BUILD].ms += t_launched - t_begin;
    if (!chain) {
        bool retry = false;
        if (int rc = B.complete(t_begin, t_launched, retry)) return rc;
        if (retry) { in_retry = true; const int rc = run(ops, tails); in_retry = false; return rc; }     // once: complete() asks only while in_retry is clear
    }
    B.mark_valid();
    if (record_plan) return B.keep_plan();
    return 0;
}

// full-traversal score of all genes from cached descriptors: refresh branch lengths / rates, then
// k_pmat + k_oplist + k_reduce exactly as run() would launch them
int Batch::replay_plan(double *lnl) {
    const double t_begin = now_ms();
    Plan &P = plan;
    HIPCHK(hipSetDevice(ctx->device));
    PmatReq *hreq = (PmatReq *)((char *)P.h + P.set.o_req);
    // Only genes whose rates (alpha) or branch lengths moved since the descriptors were last refreshed have their requests
    // visited: the device waits while this runs, and a step with nothing changed goes straight to the launches.  What tells is
    // the gene's rates epoch and its tree's length stamp (host.hpp: every writer of Tree::len renews it, a copy carries it),
    // two integer compares per gene.  (Until r06 the lengths were compared as bytes against a copy per gene, 2.4 KB for 50
    // taxa: 7 us of a C3 step with the device idle, profiles/r06_ab_step_path.txt.)
    std::vector<char> &moved = P.moved;
    moved.assign(genes.size(), 0);
    bool any_moved = false;
    for (size_t g = 0; g < genes.size(); ++g) {
        const Gene &G = genes[g];
        if (P.rates_seen[g] != G.rates_epoch) { moved[g] = 3; P.rates_seen[g] = G.rates_epoch; }
        if (P.len_seen[g] != G.tree.len_stamp) { moved[g] |= 1; P.len_seen[g] = G.tree.len_stamp; }
        any_moved = any_moved || moved[g];
    }
    if (P.check_len) for (size_t g = 0; g < genes.size(); ++g) {       // test hook: the byte compare, beside the stamps
        const auto &now = genes[g].tree.len.values();
        auto &was = P.len_copy[g];
        if (!(moved[g] & 1) && (was.size() != now.size() || std::memcmp(was.data(), now.data(), now.size() * sizeof now[0]) != 0))
            return ctx->fail(-5, "internal: branch lengths of gene " + std::to_string(g) + " changed under an unchanged length stamp");
        if (moved[g] & 1) was = now;
    }
    bool changed = false;                       // lengths and rates already on the device are not uploaded again
    if (any_moved) for (size_t i = 0; i < P.set.nreq; ++i) {
        const ReqSrc &s = P.src[i];
        if (!moved[s.gene]) continue;
        const Gene &G = genes[s.gene];
        const double t = G.tree.len[s.v][s.q];
        if (hreq[i].t != t) { hreq[i].t = t; changed = true; }
        if (moved[s.gene] & 2) { std::memcpy(hreq[i].rates, G.rates, sizeof hreq[i].rates); changed = true; }
    }
    char *ds = (char *)P.d;
    if (changed) HIPCHK(hipMemcpyAsync(ds + P.set.o_req, hreq, P.set.nreq * sizeof(PmatReq), hipMemcpyHostToDevice, ctx->stream));
    // the three launches carry their timing events themselves (profile mode): nothing but kernels in the queue
    issue(P.set, ds, true);
    if (!chain && !P.per_gene) { if (int rc = fetch_results(false)) return rc; }      // per gene: k_reduce has written h_plan_lnl itself
    const double t_launched = now_ms();
    ctx->stats[K_HOST_BUILD].launches++; ctx->stats[K_HOST_BUILD].ms += t_launched - t_begin;
    for (auto &o : P.outs) genes[o.first].valid[o.second] = 1;       // host bookkeeping while the device works
    if (!chain) {
        if (int rc = ctx->sync(ctx->stream)) return rc;
        HIPCHK(hipGetLastError());
        const double t_done = now_ms();
        ctx->stats[K_HOST_WAIT].launches++; ctx->stats[K_HOST_WAIT].ms += t_done - t_launched;
        ctx->resolve_events();
    }
    if (P.per_gene && !chain) for (size_t g = 0; g < genes.size(); ++g) res((int)g)[0] = h_plan_lnl[g];
    for (size_t g = 0; g < genes.size(); ++g) lnl[g] = res((int)g)[0];
#ifndef ABL_KEEP_GOING
    if (!chain) for (size_t g = 0; g < genes.size(); ++g) if (!std::isfinite(lnl[g])) return ctx->fail(-5, "device returned a non-finite likelihood");
#endif
    for (size_t g = 0; g < genes.size(); ++g) det_record(det_id, genes[g], 'R', 0, 0, lnl[g], genes[g].alpha, 0);
    return 0;
}

}  // namespace pml
