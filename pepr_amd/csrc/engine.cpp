// engine.cpp -- batch engine: HBM arena, lazy directional-CLV bookkeeping, level-synchronous
// newview scheduling across genes, branch-length / alpha optimisation drivers.
//
// Scheduling model (DESIGN.md "Scheduling"): every gene keeps one CLV per DIRECTED inner edge
// ("message" v->w: likelihood of the subtree hanging off v when edge (v,w) is cut).  A request
// (lnL, branch derivatives) names the messages it needs; need() walks the tree lazily and emits
// the missing newviews in dependency levels; run() uploads all descriptors of all genes once,
// launches k_pmat, one k_nv<NEWVIEW> per level, the tail kernels, and syncs once.
#include "engine.hpp"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <thread>
#include <cstring>

namespace pml {

#define HIPCHK(expr)                                                                          \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return ctx->fail(-5, std::string(#expr) + ": " + hipGetErrorString(e_));          \
    } while (0)

// ------------------------------------------------------------------------------------------
// Ctx
// ------------------------------------------------------------------------------------------
int Ctx::init(int dev, bool prof) {
    Ctx *ctx = this;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return fail(-3, "no HIP device available");
    if (dev < 0 || dev >= count) return fail(-3, "device ordinal out of range");
    device = dev; profile = prof;
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    return 0;
}
int Ctx::init_worker(const Ctx &parent) {
    Ctx *ctx = this;
    device = parent.device; profile = false;
    HIPCHK(hipSetDevice(device));
    // A stream of the HIGHEST priority class: HIP keeps a separate pool of hardware queues per priority, so the groups' streams
    // do not end up multiplexed onto a queue with each other's or the application's normal-priority streams (measured: two
    // groups on one hardware queue search 150 C3 gene-trees/s, on two queues 200, one undivided batch 175).
    int lo = 0, hi = 0;
    if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess) { lo = hi = 0; }
    if (hipStreamCreateWithPriority(&stream, hipStreamNonBlocking, hi) != hipSuccess) HIPCHK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    root = parent.root ? parent.root : &parent;
    return 0;
}
int Ctx::sync(hipStream_t s) {
    Ctx *ctx = this;
    if (!ev_sync) HIPCHK(hipEventCreateWithFlags(&ev_sync, hipEventDisableTiming));
    HIPCHK(hipEventRecord(ev_sync, s));
    HIPCHK(hipEventSynchronize(ev_sync));
    return 0;
}
void Ctx::destroy() {
    hipSetDevice(device);
    if (ev_sync) { hipEventDestroy(ev_sync); ev_sync = nullptr; }
    for (auto &e : pending) { pool.push_back(e.a); pool.push_back(e.b); }
    pending.clear();
    for (auto e : pool) hipEventDestroy(e);
    pool.clear();
    for (auto &m : shared) { hipFree(m.d_model); hipFree(m.d_eigfrags); }
    shared.clear();
    if (arena_cache) hipFree(arena_cache);
    arena_cache = nullptr; arena_cache_bytes = 0;
    if (stream && owns_stream) hipStreamDestroy(stream);
    stream = nullptr;
}
static void fill_model_dev(const Model &m, ModelDev &h) {
    std::memcpy(h.eval, m.eval, sizeof h.eval);
    std::memcpy(h.U, m.U, sizeof h.U);
    std::memcpy(h.Uinv, m.Uinv, sizeof h.Uinv);
    std::memcpy(h.pi, m.pi, sizeof h.pi);
    for (int k = 0; k < NS; ++k) for (int j = 0; j < NS; ++j) h.UinvT[j * NS + k] = m.Uinv[k * NS + j];
}
const Matrix *Ctx::matrix_of(int pm) const {
    const Ctx &r = root ? *root : *this;
    if (pm < PM_REGISTERED || (size_t)(pm - PM_REGISTERED) / 2 >= r.matrices.size()) return nullptr;
    return &r.matrices[(size_t)(pm - PM_REGISTERED) / 2];
}
std::string Ctx::model_name(int pm) const {
    if (pm == 0) return "PROTGAMMAWAG";
    if (pm == 1) return "PROTGAMMAWAG (full-precision frequencies)";
    if (pm == 2) return "PROTGAMMAWAGF";
    if (pm == PM_GTR) return "PROTGAMMAGTR";
    const Matrix *m = matrix_of(pm);
    if (!m) return "model code " + std::to_string(pm);
    std::string n = "PROTGAMMA";
    for (char ch : m->name) n += (char)std::toupper((unsigned char)ch);
    return (pm & 1) ? n + "F" : n;
}
// One eigen-system per shared code and context.  The built-in WAG codes are decomposed on the host (the bits they always
// had); a registered matrix goes through k_model like every other model that is not built in.
int Ctx::ensure_model(int pm) {
    Ctx *ctx = this;
    if (!valid_code(pm)) return fail(-1, "bad pi_mode " + std::to_string(pm) + " (not a built-in model and not a registered matrix)");
    if (model_per_gene(pm) || shared_of(pm)) return 0;      // per-gene models live in the batch (Batch::build_gene_models)
    Shared sh{pm, nullptr, nullptr};
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipMalloc((void **)&sh.d_model, sizeof(ModelDev)));
    HIPCHK(hipMalloc((void **)&sh.d_eigfrags, sizeof(double) * 2 * PFRAG));
    if (const Matrix *M = matrix_of(pm)) {
        struct In { double exch[NEXCH], pi[NS]; ModelReq req; } h, *d = nullptr;
        std::memcpy(h.exch, M->exch, sizeof h.exch); std::memcpy(h.pi, M->pi, sizeof h.pi);
        HIPCHK(hipMalloc((void **)&d, sizeof(In)));
        h.req = ModelReq{d->exch, d->pi, sh.d_model, -1, 0.0};
        HIPCHK(hipMemcpy(d, &h, sizeof h, hipMemcpyHostToDevice));
        Ev ev = tic_self(K_MODEL, sizeof(ModelDev));
        launch_model_build(&d->req, 1, stream, ev.a, ev.b);
        if (int rc = sync(stream)) return rc;
        HIPCHK(hipFree(d));
    } else {
        Model m; m.init(pm);
        ModelDev h;
        fill_model_dev(m, h);
        HIPCHK(hipMemcpy(sh.d_model, &h, sizeof h, hipMemcpyHostToDevice));
    }
    launch_eigfrags(sh.d_model, sh.d_eigfrags, stream);
    if (int rc = sync(stream)) return rc;
    HIPCHK(hipGetLastError());
    shared.push_back(sh);
    return 0;
}

// ------------------------------------------------------------------------------------------
// per-gene models
// ------------------------------------------------------------------------------------------
int Batch::alloc_gene_models() {
    const size_t n = genes.size();
    HIPCHK(hipMalloc((void **)&d_gmodel, n * sizeof(ModelDev)));
    HIPCHK(hipMalloc((void **)&d_geig, n * 2 * PFRAG * sizeof(double)));
    HIPCHK(hipMalloc((void **)&d_gexch, n * NEXCH * sizeof(double)));
    HIPCHK(hipMalloc((void **)&d_gpi, n * NS * sizeof(double)));
    HIPCHK(hipMalloc((void **)&d_mreq, n * sizeof(ModelReq)));
    HIPCHK(hipHostMalloc((void **)&h_gexch, n * NEXCH * sizeof(double), hipHostMallocDefault));
    HIPCHK(hipHostMalloc((void **)&h_gpi, n * NS * sizeof(double), hipHostMallocDefault));
    HIPCHK(hipHostMalloc((void **)&h_mreq, n * sizeof(ModelReq), hipHostMallocDefault));
    return 0;
}
void Batch::empirical_pi(int g, double *pi) const {
    if (genes[g].counted_pi.empty()) empirical_freqs(genes[g].aln, pi);
    else std::memcpy(pi, genes[g].counted_pi.data(), sizeof(double) * NS);
}
void Batch::matrix_for(int g, double *exch, double *pi) const {
    const int code = genes[g].model_code;
    const Matrix *M = ctx->matrix_of(code);
    std::memcpy(exch, M ? M->exch : wag_exch(), sizeof(double) * NEXCH);
    // GTR starts from WAG in the scale the estimates are reported in: the last exchangeability, which stays fixed, is 1
    if (code == PM_GTR) { const double last = exch[NEXCH - 1]; for (int i = 0; i < NEXCH; ++i) exch[i] /= last; }
    if (model_per_gene(code)) empirical_pi(g, pi);
    else std::memcpy(pi, M ? M->pi : wag_pi(code), sizeof(double) * NS);
    double sum = 0;
    for (int i = 0; i < NS; ++i) sum += pi[i];
    for (int i = 0; i < NS; ++i) pi[i] /= sum;
}
// Every gene gets its own ModelDev and eigen-basis fragment sets.  A gene of a shared code receives a copy of the context's
// model (the same bytes, hence the same results as in a shared-model batch); PROTGAMMAWAGF (code 2) is decomposed on the
// host as it always was; every other per-gene code (registered "F" variants, GTR from its WAG start) is built by k_model.
int Batch::build_gene_models() {
    const int n = (int)genes.size();
    if (int rc = alloc_gene_models()) return rc;
    std::vector<ModelDev> h(n);
    std::vector<int> dev;
    for (int g = 0; g < n; ++g) {
        const int code = genes[g].model_code;
        if (code == 2) {
            double pi[NS];
            empirical_pi(g, pi);
            Model m; m.init_pi(pi);
            fill_model_dev(m, h[g]);
            std::memcpy(h_gexch + (size_t)g * NEXCH, wag_exch(), sizeof(double) * NEXCH); std::memcpy(h_gpi + (size_t)g * NS, m.pi, sizeof m.pi);
            HIPCHK(hipMemcpyAsync(d_gmodel + g, &h[g], sizeof(ModelDev), hipMemcpyHostToDevice, ctx->stream));
            continue;
        }
        matrix_for(g, h_gexch + (size_t)g * NEXCH, h_gpi + (size_t)g * NS);
        if (model_per_gene(code)) { dev.push_back(g); continue; }
        if (int rc = ctx->ensure_model(code)) return rc;
        HIPCHK(hipMemcpyAsync(d_gmodel + g, ctx->shared_of(code)->d_model, sizeof(ModelDev), hipMemcpyDeviceToDevice, ctx->stream));
    }
    HIPCHK(hipMemcpyAsync(d_gexch, h_gexch, (size_t)n * NEXCH * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(d_gpi, h_gpi, (size_t)n * NS * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if (int rc = build_models(dev, -1, nullptr)) return rc;          // ends with the fragment sets of ALL genes
    if (dev.empty()) launch_eigfrags_n(d_gmodel, d_geig, n, ctx->stream);
    if (int rc = ctx->sync(ctx->stream)) return rc;      // h goes out of scope
    HIPCHK(hipGetLastError());
    return 0;
}
// h_mreq is reused by the next call: every caller synchronises the stream (a score, or explicitly) before it calls again.
// PML_MODEL_HOST=1 is the A/B arm this kernel is judged against: the same models decomposed one after the
// other on the host (Model::init) and uploaded.
int Batch::build_models(const std::vector<int> &gs, int patch, const double *vals) {
    if (gs.empty()) return 0;
    static const bool host_arm = std::getenv("PML_MODEL_HOST") != nullptr;
    const int n = (int)genes.size(), m = (int)gs.size();
    if (host_arm) {
        if (!h_gmodel) HIPCHK(hipHostMalloc((void **)&h_gmodel, (size_t)n * sizeof(ModelDev), hipHostMallocDefault));
        for (int i = 0; i < m; ++i) {
            const int g = gs[i];
            double ex[NEXCH];
            std::memcpy(ex, h_gexch + (size_t)g * NEXCH, sizeof ex);
            if (patch >= 0) ex[patch] = vals[i];
            Model md; md.init(ex, h_gpi + (size_t)g * NS);
            fill_model_dev(md, h_gmodel[g]);
            HIPCHK(hipMemcpyAsync(d_gmodel + g, h_gmodel + g, sizeof(ModelDev), hipMemcpyHostToDevice, ctx->stream));
        }
    } else {
        for (int i = 0; i < m; ++i) {
            const int g = gs[i];
            h_mreq[i] = ModelReq{d_gexch + (size_t)g * NEXCH, d_gpi + (size_t)g * NS, d_gmodel + g, patch, patch >= 0 ? vals[i] : 0.0};
        }
        HIPCHK(hipMemcpyAsync(d_mreq, h_mreq, (size_t)m * sizeof(ModelReq), hipMemcpyHostToDevice, ctx->stream));
        Ctx::Ev ev = ctx->tic_self(K_MODEL, (double)m * sizeof(ModelDev));
        launch_model_build(d_mreq, m, ctx->stream, ev.a, ev.b);
    }
    launch_eigfrags_n(d_gmodel, d_geig, n, ctx->stream);
    return 0;
}
// A model change counts as a move of every branch of the gene: its cached CLVs are invalid, and a recorded scoring plan
// recomputes all its transition matrices from the rebuilt ModelDev at the next replay (k_pmat reads the model through the
// request's pointer on every replay).  A batch created with a shared model becomes a per-gene batch here: every gene gets a
// copy of the shared model first, and a recorded plan -- whose requests name no model -- is dropped.
int Batch::set_matrix(int g, const double *exch, const double *pi) {
    const int n = (int)genes.size();
    HIPCHK(hipSetDevice(ctx->device));
    if (!d_gmodel) {
        if (int rc = alloc_gene_models()) return rc;
        for (int i = 0; i < n; ++i) {
            matrix_for(i, h_gexch + (size_t)i * NEXCH, h_gpi + (size_t)i * NS);
            HIPCHK(hipMemcpyAsync(d_gmodel + i, d_shared, sizeof(ModelDev), hipMemcpyDeviceToDevice, ctx->stream));
            HIPCHK(hipMemcpyAsync(d_geig + (size_t)i * 2 * PFRAG, d_shared_eig, sizeof(double) * 2 * PFRAG, hipMemcpyDeviceToDevice, ctx->stream));
        }
        plan.valid = false;
    }
    std::vector<int> gs;
    for (int i = 0; i < n; ++i) if (g < 0 || i == g) gs.push_back(i);
    for (int i : gs) {
        std::memcpy(h_gexch + (size_t)i * NEXCH, exch, sizeof(double) * NEXCH);
        if (pi) {
            double sum = 0;
            for (int k = 0; k < NS; ++k) sum += pi[k];
            for (int k = 0; k < NS; ++k) h_gpi[(size_t)i * NS + k] = pi[k] / sum;
        }
        invalidate_all(i);
    }
    HIPCHK(hipMemcpyAsync(d_gexch, h_gexch, (size_t)n * NEXCH * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(d_gpi, h_gpi, (size_t)n * NS * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if (int rc = build_models(gs, -1, nullptr)) return rc;
    if (int rc = ctx->sync(ctx->stream)) return rc;
    HIPCHK(hipGetLastError());
    return 0;
}
int Batch::get_matrix(int g, double *exch, double *pi) const {
    if (h_gexch) {
        if (exch) std::memcpy(exch, h_gexch + (size_t)g * NEXCH, sizeof(double) * NEXCH);
        if (pi) std::memcpy(pi, h_gpi + (size_t)g * NS, sizeof(double) * NS);
        return 0;
    }
    double ex[NEXCH], p[NS];
    matrix_for(g, ex, p);
    if (exch) std::memcpy(exch, ex, sizeof ex);
    if (pi) std::memcpy(pi, p, sizeof p);
    return 0;
}
hipEvent_t Ctx::get_event() {
    if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
    hipEvent_t e; hipEventCreate(&e); return e;
}
void Ctx::tic(int kind, double bytes, double flops) {
    stats[kind].launches++; stats[kind].bytes += bytes; stats[kind].flops += flops;
    if (!profile) return;
    Ev ev{kind, get_event(), get_event()};
    hipEventRecord(ev.a, stream);
    pending.push_back(ev);
}
void Ctx::toc() {
    if (!profile) return;
    hipEventRecord(pending.back().b, stream);
}
Ctx::Ev Ctx::tic_self(int kind, double bytes, double flops) {
    stats[kind].launches++; stats[kind].bytes += bytes; stats[kind].flops += flops;
    if (!profile) return Ev{kind, nullptr, nullptr};
    pending.push_back(Ev{kind, get_event(), get_event()});
    return pending.back();
}
void Ctx::resolve_events() {
    for (auto &e : pending) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, e.a, e.b) == hipSuccess) stats[e.kind].ms += ms;
        pool.push_back(e.a); pool.push_back(e.b);
    }
    pending.clear();
}

// ------------------------------------------------------------------------------------------
// Batch: creation / layout
// ------------------------------------------------------------------------------------------

// PML_DET_LOG=<file>: every value the host consumes from the device (evaluations, Newton results) is recorded in memory
// as a binary record and written out at process exit -- a determinism diagnostic (tools/dbg_detlog_diff.py) whose cost per
// record is a few stores, so it does not perturb the timing it is meant to observe; off unless the variable is set
struct DetRec { int batch, ntax, npat, nsites, kind, a, b, pad; double x, y, z; };
static std::vector<DetRec> *g_det = nullptr;
static std::mutex g_det_mu;
static bool det_on() {
    static const bool on = [] {
        const char *p = std::getenv("PML_DET_LOG");
        if (!p) return false;
        g_det = new std::vector<DetRec>(); g_det->reserve(1 << 22);
        std::atexit([] {
            const char *q = std::getenv("PML_DET_LOG"); FILE *f = q ? std::fopen(q, "w") : nullptr;
            if (!f) return;
            for (const DetRec &r : *g_det) std::fprintf(f, "B%d g%d_%d_%d %c %d %d %a %a %a\n", r.batch, r.ntax, r.npat, r.nsites, (char)r.kind, r.a, r.b, r.x, r.y, r.z);
            std::fclose(f);
        });
        return true;
    }();
    return on;
}
void det_record(int batch, const Gene &G, char kind, int a, int b, double x, double y, double z) {
    if (!det_on()) return;
    std::lock_guard<std::mutex> lk(g_det_mu);
    g_det->push_back(DetRec{batch, G.aln.ntax, G.aln.npat, G.aln.nsites, kind, a, b, 0, x, y, z});
}
static std::atomic<int> g_batch_id{0};

int Batch::create(Ctx *c, int n, const pml_alignment_view *alns, const char *const *newicks, int pm, int nc,
                  double alpha, bool score_only, const int *gene_codes) {
    ctx = c; pi_mode = pm; ncat = nc; score_only_batch = score_only;
    det_id = ++g_batch_id;
    virtual_cherries = std::getenv("PML_NO_CHERRY") == nullptr;
    virtual_pitch = virtual_cherries && std::getenv("PML_NO_PITCH") == nullptr;
    if (n <= 0) return ctx->fail(-1, "empty batch");
    if (nc != 1 && nc != 4) return ctx->fail(-1, "ncat must be 1 or 4");
    if (gene_codes) { for (int g = 0; g < n; ++g) if (!ctx->valid_code(gene_codes[g])) return ctx->fail(-1, "bad pi_mode " + std::to_string(gene_codes[g])); }
    else if (int rc = ctx->ensure_model(pm)) return rc;
    const bool per_gene = gene_codes != nullptr || model_per_gene(pm);
    if (!per_gene) { d_shared = ctx->shared_of(pm)->d_model; d_shared_eig = ctx->shared_of(pm)->d_eigfrags; }
    HIPCHK(hipSetDevice(ctx->device));
    genes.resize(n);
    for (int g = 0; g < n; ++g) genes[g].model_code = gene_codes ? gene_codes[g] : pm;
    const double t_create0 = now_ms();
    {   // encode / parse / NJ are independent per gene: host threads (plain std::thread, no GPU work)
        const int nthreads = std::max(1, std::min({n, 16, (int)std::thread::hardware_concurrency()}));
        std::vector<std::string> errs(n);
        std::atomic<int> next{0};
        auto work = [&]() {
            for (int g = next++; g < n; g = next++) {
                Gene &G = genes[g];
                try {
                    if (!G.aln.encode(alns[g].ntax, alns[g].nsites, alns[g].names, alns[g].rows, errs[g])) continue;
                    if (newicks && newicks[g]) { if (!Tree::parse(newicks[g], G.aln.names, G.tree, errs[g])) continue; }
                    else G.tree = nj_tree(G.aln);
                } catch (const std::exception &e) { errs[g] = e.what(); }
            }
        };
        std::vector<std::thread> pool;
        for (int t = 1; t < nthreads; ++t) pool.emplace_back(work);
        work();
        for (auto &t : pool) t.join();
        for (int g = 0; g < n; ++g) if (!errs[g].empty()) return ctx->fail(-2, "gene " + std::to_string(g) + ": " + errs[g]);
    }
    if (std::getenv("PML_TRACE")) fprintf(stderr, "[pml] create: encode + start trees of %d genes %.1f ms\n", n, now_ms() - t_create0);
    if (int rc = layout(alpha, score_only)) return rc;
    return per_gene ? build_gene_models() : 0;
}

// device arena + per-gene pointers from (ntax, mpad) alone; host-encoded codes/weights are uploaded when present
// (replicates built by create_replicates() have none: k_gather fills them)
int Batch::layout(double alpha, bool score_only) {
    const int n = (int)genes.size();
    size_t total = 0;
    std::vector<size_t> off(n);
    for (int g = 0; g < n; ++g) {
        Gene &G = genes[g];
        const int nt = G.aln.ntax, mp = G.aln.mpad, ndir = 3 * (nt - 2);
        G.slot_cap = score_only ? (nt - 2) : ndir;
        // a search2 batch: SPR path CLVs for every depth the gene's taxon count can reach, + insertion slot + one spare
        G.nscratch = std::max(NSCRATCH, std::min(spr_scratch_radius, nt) + 2);
        G.slot_of.assign(ndir, -1); G.valid.assign(ndir, 0); G.pend_level.assign(ndir, -1);
        G.mark_all();
        off[g] = total;
        total += align_up((size_t)nt * mp, 256);                       // codes
        total += align_up((size_t)mp * 8, 256);                        // weight
        total += (size_t)(G.slot_cap + G.nscratch) * clv_doubles(mp) * 8;  // clv (+ scratch), tiled: whole 128-pattern tiles
        total += align_up((size_t)(G.slot_cap + G.nscratch) * mp * 4, 256);   // scalers
        total += (size_t)MAXTAIL * clv_doubles(mp) * 8;                  // sumtables
        total += (size_t)MAXTAIL * align_up((size_t)mp * 4, 256);      // sumtable scalers
        total += (size_t)MAXTAIL * align_up((size_t)mp * 8, 256);      // per-pattern lnL
    }
    arena_bytes = total;
    const double t_alloc0 = now_ms();
    if (ctx->arena_cache && ctx->arena_cache_bytes >= total) {        // reuse: no driver allocation, no zero-fill
        arena = ctx->arena_cache; arena_bytes = ctx->arena_cache_bytes;
        ctx->arena_cache = nullptr; ctx->arena_cache_bytes = 0;
    } else {
        if (ctx->arena_cache) { hipFree(ctx->arena_cache); ctx->arena_cache = nullptr; ctx->arena_cache_bytes = 0; }
        if (hipMalloc((void **)&arena, total) != hipSuccess) {
            arena = nullptr;
            return ctx->fail(-4, "device arena of " + std::to_string(total >> 20) + " MiB does not fit");
        }
    }
    // debugging aid: a reused arena holds stale data; poisoning it (all-ones = NaN doubles, -1 counts) makes any read of
    // a location this batch has not written show up in the results
    if (std::getenv("PML_POISON_ARENA")) HIPCHK(hipMemsetAsync(arena, 0xFF, total, ctx->stream));
    for (int g = 0; g < n; ++g) {
        Gene &G = genes[g];
        const int nt = G.aln.ntax, mp = G.aln.mpad;
        char *p = arena + off[g];
        G.d_codes = (uint8_t *)p; p += align_up((size_t)nt * mp, 256);
        G.d_weight = (double *)p; p += align_up((size_t)mp * 8, 256);
        G.d_clv = (double *)p; p += (size_t)(G.slot_cap + G.nscratch) * clv_doubles(mp) * 8;
        G.d_scl = (int *)p; p += align_up((size_t)(G.slot_cap + G.nscratch) * mp * 4, 256);
        for (int k = 0; k < MAXTAIL; ++k) { G.d_sumtab[k] = (double *)p; p += clv_doubles(mp) * 8; }
        for (int k = 0; k < MAXTAIL; ++k) { G.d_sumscl[k] = (int *)p; p += align_up((size_t)mp * 4, 256); }
        for (int k = 0; k < MAXTAIL; ++k) { G.d_patlnl[k] = (double *)p; p += align_up((size_t)mp * 8, 256); }
        if (!G.aln.codes.empty()) {
            HIPCHK(hipMemcpyAsync(G.d_codes, G.aln.codes.data(), (size_t)nt * mp, hipMemcpyHostToDevice, ctx->stream));
            HIPCHK(hipMemcpyAsync(G.d_weight, G.aln.weight.data(), (size_t)mp * 8, hipMemcpyHostToDevice, ctx->stream));
        }
        set_alpha(g, alpha);
    }
    // results (8 doubles per gene) are written by the kernels straight into mapped pinned host
    // memory: no device-to-host copy node per step
    // Results (8 doubles per gene and tail slot) live in DEVICE memory and reach the host by an explicit copy on the engine's
    // stream before every synchronisation (fetch_results).  Rounds 1-2 let the kernels store them straight into mapped host
    // memory; the explicit copy keeps PCIe writes out of the kernels and makes the hand-over an ordinary stream operation
    // (it was one of the suspects of the reproducibility hunt of DESIGN.md 9 r02-g and changed nothing there).
    scalars_doubles = (size_t)8 * MAXTAIL * n;
    HIPCHK(hipMalloc((void **)&d_scalars, sizeof(double) * scalars_doubles));
    HIPCHK(hipHostMalloc((void **)&h_scalars, sizeof(double) * scalars_doubles, hipHostMallocDefault));
    std::memset(h_scalars, 0, sizeof(double) * scalars_doubles);
    // The exception: a replayed scoring plan (replay_plan) produces one lnL per gene, and its k_reduce stores that double
    // straight into mapped, coherent pinned memory -- one 8-byte write per gene at the end of the step instead of a copy
    // operation queued behind the kernel; the host reads it after the event that follows k_reduce has completed.
    HIPCHK(hipHostMalloc((void **)&h_plan_lnl, sizeof(double) * n, hipHostMallocMapped | hipHostMallocCoherent));
    HIPCHK(hipHostGetDevicePointer((void **)&d_plan_lnl, h_plan_lnl, 0));
    { if (int rc_ = ctx->sync(ctx->stream)) return rc_; }
    if (std::getenv("PML_TRACE")) fprintf(stderr, "[pml] layout: arena %.1f GiB allocated + uploaded in %.1f ms\n", (double)total / (1 << 30), now_ms() - t_alloc0);
    return 0;
}

void Batch::destroy() {
    if (!ctx) return;
    hipSetDevice(ctx->device);
    if (arena) {
        if (ctx->arena_cache_bytes < arena_bytes) {                  // keep the larger one for the next batch
            if (ctx->arena_cache) hipFree(ctx->arena_cache);
            ctx->arena_cache = arena; ctx->arena_cache_bytes = arena_bytes;
        } else hipFree(arena);
    }
    if (h_stage) hipHostFree(h_stage);
    if (d_stage) hipFree(d_stage);
    if (d_frags) hipFree(d_frags);
    if (d_nsync) hipFree(d_nsync);
    if (d_nctl) {
        if (std::getenv("PML_TRACE")) {
            NewtonCtl h;
            if (hipMemcpy(&h, d_nctl, sizeof h, hipMemcpyDeviceToHost) == hipSuccess && h.n_requests)
                fprintf(stderr, "[pml] branch Newton: %llu requests, %.2f evaluations each\n", h.n_requests, (double)h.n_evals / (double)h.n_requests);
        }
        hipFree(d_nctl); d_nctl = nullptr;
    }
    if (d_gmodel) { hipFree(d_gmodel); d_gmodel = nullptr; }
    if (d_geig) { hipFree(d_geig); d_geig = nullptr; }
    if (d_gexch) { hipFree(d_gexch); d_gexch = nullptr; }
    if (d_gpi) { hipFree(d_gpi); d_gpi = nullptr; }
    if (d_mreq) { hipFree(d_mreq); d_mreq = nullptr; }
    if (h_gexch) { hipHostFree(h_gexch); h_gexch = nullptr; }
    if (h_gpi) { hipHostFree(h_gpi); h_gpi = nullptr; }
    if (h_mreq) { hipHostFree(h_mreq); h_mreq = nullptr; }
    if (h_gmodel) { hipHostFree(h_gmodel); h_gmodel = nullptr; }
    d_nsync = nullptr; nsync_cap = 0;
    if (plan.h) hipHostFree(plan.h);
    if (plan.d) hipFree(plan.d);
    plan = Plan();
    if (h_scalars) hipHostFree(h_scalars);
    if (d_scalars) hipFree(d_scalars);
    if (h_plan_lnl) hipHostFree(h_plan_lnl);
    h_plan_lnl = d_plan_lnl = nullptr;
    if (h_chain) hipHostFree(h_chain);
    if (d_chain) hipFree(d_chain);
    if (d_lenpool) hipFree(d_lenpool);
    if (d_tailpool) { hipFree(d_tailpool); d_tailpool = nullptr; tailpool_cap = 0; }
    if (d_site2pat) { hipFree(d_site2pat); d_site2pat = nullptr; }
    h_chain = d_chain = nullptr; d_lenpool = nullptr; chain_cap = 0;
    arena = nullptr; h_stage = d_stage = nullptr; d_frags = nullptr; d_scalars = h_scalars = nullptr;
}

// ------------------------------------------------------------------------------------------
// GeneStore / create_replicates: jackknife concatenation on the device
// ------------------------------------------------------------------------------------------
int GeneStore::create(Ctx *c, int n, const pml_alignment_view *alns) {
    ctx = c;
    HIPCHK(hipSetDevice(ctx->device));
    items.resize(n);
    std::vector<std::string> errs(n);
    std::atomic<int> next{0};
    auto work = [&]() {
        for (int g = next++; g < n; g = next++) {
            try { if (items[g].aln.encode(alns[g].ntax, alns[g].nsites, alns[g].names, alns[g].rows, errs[g])) pair_counts(items[g].aln, items[g].cmp, items[g].diff); }
            catch (const std::exception &e) { errs[g] = e.what(); }
        }
    };
    const int nthreads = std::max(1, std::min({n, 16, (int)std::thread::hardware_concurrency()}));
    std::vector<std::thread> pool;
    for (int t = 1; t < nthreads; ++t) pool.emplace_back(work);
    work();
    for (auto &t : pool) t.join();
    for (int g = 0; g < n; ++g) if (!errs[g].empty()) return ctx->fail(-2, "gene " + std::to_string(g) + ": " + errs[g]);
    size_t total = 0;
    for (auto &it : items) total += align_up((size_t)it.aln.ntax * it.aln.mpad, 256) + align_up((size_t)it.aln.mpad * 8, 256);
    if (hipMalloc((void **)&arena, total) != hipSuccess) { arena = nullptr; return ctx->fail(-4, "gene store does not fit on the device"); }
    char *p = arena;
    for (auto &it : items) {
        it.d_codes = (uint8_t *)p; p += align_up((size_t)it.aln.ntax * it.aln.mpad, 256);
        it.d_w = (double *)p; p += align_up((size_t)it.aln.mpad * 8, 256);
        HIPCHK(hipMemcpyAsync(it.d_codes, it.aln.codes.data(), (size_t)it.aln.ntax * it.aln.mpad, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(hipMemcpyAsync(it.d_w, it.aln.weight.data(), (size_t)it.aln.mpad * 8, hipMemcpyHostToDevice, ctx->stream));
    }
    { if (int rc_ = ctx->sync(ctx->stream)) return rc_; }
    return 0;
}
void GeneStore::destroy() { if (arena) { hipSetDevice(ctx->device); hipFree(arena); arena = nullptr; } items.clear(); }

int Batch::create_replicates(Ctx *c, const GeneStore &store, const std::vector<std::vector<int>> &sel, int pm, int nc, double alpha) {
    ctx = c; pi_mode = pm; ncat = nc; score_only_batch = false;
    virtual_cherries = std::getenv("PML_NO_CHERRY") == nullptr;
    virtual_pitch = virtual_cherries && std::getenv("PML_NO_PITCH") == nullptr;
    const int n = (int)sel.size();
    if (n <= 0) return ctx->fail(-1, "empty batch");
    if (int rc = ctx->ensure_model(pm)) return rc;                 // also refuses an unknown code
    const bool per_gene = model_per_gene(pm);
    if (!per_gene) { d_shared = ctx->shared_of(pm)->d_model; d_shared_eig = ctx->shared_of(pm)->d_eigfrags; }
    HIPCHK(hipSetDevice(ctx->device));
    genes.resize(n);
    for (auto &G : genes) G.model_code = pm;
    struct SegH { int rep, gene, off; size_t rowmap_off; };
    std::vector<SegH> segs; std::vector<int> rowmaps;
    int max_npat = 0;
    for (int r = 0; r < n; ++r) {
        Gene &G = genes[r]; EncodedAlignment &A = G.aln;
        std::vector<std::string> names;
        for (int g : sel[r]) {
            if (g < 0 || g >= (int)store.items.size()) return ctx->fail(-1, "gene index out of range");
            names.insert(names.end(), store.items[g].aln.names.begin(), store.items[g].aln.names.end());
        }
        std::sort(names.begin(), names.end()); names.erase(std::unique(names.begin(), names.end()), names.end());   // MSAConcatenator.java:78-189: sorted union
        const int nt = (int)names.size();
        if (nt < 3) return ctx->fail(-2, "replicate " + std::to_string(r) + ": fewer than 3 taxa");
        A.ntax = nt; A.names = names; A.nsites = 0; A.npat = 0;
        std::vector<int64_t> cmp((size_t)nt * nt, 0), diff((size_t)nt * nt, 0);
        for (int g : sel[r]) {
            const GeneStore::Item &it = store.items[g];
            std::vector<int> local(it.aln.ntax);                 // gene row -> replicate row
            SegH sh{r, g, A.npat, rowmaps.size()};
            rowmaps.resize(rowmaps.size() + nt, -1);
            for (int i = 0; i < it.aln.ntax; ++i) {
                local[i] = (int)(std::lower_bound(names.begin(), names.end(), it.aln.names[i]) - names.begin());
                rowmaps[sh.rowmap_off + local[i]] = i;
            }
            for (int i = 0; i < it.aln.ntax; ++i) for (int j = 0; j < it.aln.ntax; ++j) {
                cmp[(size_t)local[i] * nt + local[j]] += it.cmp[(size_t)i * it.aln.ntax + j]; diff[(size_t)local[i] * nt + local[j]] += it.diff[(size_t)i * it.aln.ntax + j];
            }
            segs.push_back(sh);
            A.npat += it.aln.npat; A.nsites += it.aln.nsites; max_npat = std::max(max_npat, it.aln.npat);
        }
        A.mpad = (A.npat + 31) / 32 * 32;
        G.tree = nj_from_counts(nt, cmp, diff);
    }
    if (int rc = layout(alpha, false)) return rc;
    // padding patterns: gap code, weight 0; then one gather launch fills every replicate
    for (auto &G : genes) {
        HIPCHK(hipMemsetAsync(G.d_codes, NCODES - 1, (size_t)G.aln.ntax * G.aln.mpad, ctx->stream));
        HIPCHK(hipMemsetAsync(G.d_weight, 0, (size_t)G.aln.mpad * 8, ctx->stream));
    }
    std::vector<GatherSeg> hs(segs.size());
    void *d_buf = nullptr;
    const size_t seg_bytes = align_up(hs.size() * sizeof(GatherSeg), 256), map_bytes = rowmaps.size() * sizeof(int);
    HIPCHK(hipMalloc(&d_buf, seg_bytes + map_bytes));
    const int *d_maps = (const int *)((char *)d_buf + seg_bytes);
    for (size_t i = 0; i < segs.size(); ++i) {
        const GeneStore::Item &it = store.items[segs[i].gene]; Gene &G = genes[segs[i].rep];
        hs[i] = GatherSeg{it.d_codes, it.d_w, G.d_codes, G.d_weight, d_maps + segs[i].rowmap_off, it.aln.mpad, it.aln.npat, G.aln.mpad, segs[i].off, G.aln.ntax, 0};
    }
    hipError_t e1 = hipMemcpyAsync(d_buf, hs.data(), hs.size() * sizeof(GatherSeg), hipMemcpyHostToDevice, ctx->stream);
    hipError_t e2 = hipMemcpyAsync((char *)d_buf + seg_bytes, rowmaps.data(), map_bytes, hipMemcpyHostToDevice, ctx->stream);
    if (e1 == hipSuccess && e2 == hipSuccess) launch_gather((const GatherSeg *)d_buf, (int)hs.size(), max_npat, ctx->stream);
    hipError_t e3 = ctx->sync(ctx->stream) ? hipErrorUnknown : hipSuccess;
    hipFree(d_buf);
    if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess) return ctx->fail(-4, "replicate gather failed");
    if (!per_gene) return 0;
    // a model per replicate, as Batch::create builds one per gene: the frequencies come from the gathered matrix itself
    if (int rc = count_replicate_freqs()) return rc;
    return build_gene_models();
}

int Batch::count_replicate_freqs() {
    const int n = (int)genes.size();
    const size_t req_bytes = align_up((size_t)n * sizeof(CodeHistReq), 256), out_bytes = (size_t)n * NCODES * sizeof(long long);
    std::vector<CodeHistReq> hr((size_t)n);
    std::vector<long long> hist((size_t)n * NCODES);
    int max_mpad = 0;
    for (int g = 0; g < n; ++g) { const Gene &G = genes[g]; hr[g] = CodeHistReq{G.d_codes, G.d_weight, G.aln.ntax, G.aln.mpad}; max_mpad = std::max(max_mpad, G.aln.mpad); }
    char *d_buf = nullptr;
    HIPCHK(hipMalloc((void **)&d_buf, req_bytes + out_bytes));
    long long *d_out = (long long *)(d_buf + req_bytes);
    size_t cells = 0;
    for (auto &G : genes) cells += (size_t)G.aln.ntax * G.aln.mpad;
    hipError_t e = hipMemcpyAsync(d_buf, hr.data(), (size_t)n * sizeof(CodeHistReq), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(d_out, 0, out_bytes, ctx->stream);
    if (e == hipSuccess) {
        ctx->tic(K_CODEHIST, (double)cells);
        launch_codehist((const CodeHistReq *)d_buf, n, max_mpad, d_out, ctx->stream);
        ctx->toc();
        e = hipMemcpyAsync(hist.data(), d_out, out_bytes, hipMemcpyDeviceToHost, ctx->stream);
    }
    if (e == hipSuccess && ctx->sync(ctx->stream)) e = hipErrorUnknown;
    if (e == hipSuccess) e = hipGetLastError();
    hipFree(d_buf);
    if (e != hipSuccess) return ctx->fail(-4, std::string("code histogram of the replicates failed: ") + hipGetErrorString(e));
    for (int g = 0; g < n; ++g) {
        Gene &G = genes[g];
        G.code_hist.assign(hist.begin() + (size_t)g * NCODES, hist.begin() + (size_t)(g + 1) * NCODES);
        G.counted_pi.resize(NS);
        empirical_freqs_from_counts(G.code_hist.data(), G.counted_pi.data());
    }
    return 0;
}

void Batch::set_alpha(int g, double a) {
    Gene &G = genes[g];
    a = std::min(std::max(a, ALPHA_MIN), ALPHA_MAX);
    G.alpha = a;
    if (ncat == 1) { for (double &r : G.rates) r = 1.0; }
    else gamma_rates(a, NCAT, G.rates);
    ++G.rates_epoch;
    invalidate_all(g);
}
void Batch::invalidate_all(int g) {
    Gene &G = genes[g];
    std::fill(G.valid.begin(), G.valid.end(), 0);
    if (G.slot_cap < (int)G.slot_of.size()) { std::fill(G.slot_of.begin(), G.slot_of.end(), -1); G.next_slot = 0; }
}
static void invalidate_from(Gene &G, int v, int from) {
    // iterative DFS: every message leaving v away from `from`, and onwards
    std::vector<std::pair<int, int>> st{{v, from}};
    const int nt = G.aln.ntax;
    while (!st.empty()) {
        auto [x, f] = st.back(); st.pop_back();
        if (x < nt) continue;
        for (int k = 0; k < 3; ++k) {
            const int w = G.tree.nbr[x][k];
            if (w == f || w < 0) continue;
            G.valid[(x - nt) * 3 + k] = 0;
            st.push_back({w, x});
        }
    }
}
void Batch::branch_changed(int g, int a, int b) {
    invalidate_from(genes[g], a, b); invalidate_from(genes[g], b, a);
}
int Batch::slot_for(Gene &G, int idx) {
    int s = G.slot_of[idx];
    if (s < 0) { if (G.next_slot >= G.slot_cap) return -1; s = G.slot_of[idx] = G.next_slot++; }
    return s;
}

// ------------------------------------------------------------------------------------------
// lazy collection of the newviews a message depends on
// ------------------------------------------------------------------------------------------
bool Batch::is_cherry(int g, int node, int toward) const {
    const Gene &G = genes[g];
    const int nt = G.aln.ntax;
    if (!virtual_cherries || node < nt) return false;
    for (int k = 0; k < 3; ++k) { const int w = G.tree.nbr[node][k]; if (w != toward && w >= nt) return false; }
    return true;
}
int Batch::virt_kind(int g, int node, int toward) const {
    if (is_cherry(g, node, toward)) return 1;
    if (!virtual_pitch) return 0;
    const Gene &G = genes[g];
    const int nt = G.aln.ntax;
    if (node < nt) return 0;
    int ntip = 0, inner = -1;
    for (int k = 0; k < 3; ++k) { const int w = G.tree.nbr[node][k]; if (w == toward) continue; if (w < nt) ++ntip; else inner = w; }
    return (ntip == 1 && inner >= 0 && is_cherry(g, inner, node)) ? 2 : 0;
}
Side Batch::msg(int g, int node, int toward) const {
    const Gene &G = genes[g];
    if (node < G.aln.ntax) return {SIDE_TIP, node};
    const int idx = (node - G.aln.ntax) * 3 + G.tree.slot(node, toward);
    const int vk = virt_kind(g, node, toward);
    return {vk == 1 ? SIDE_CHERRY : (vk == 2 ? SIDE_PITCH : SIDE_MSG), idx};
}

int Batch::need(int g, int v, int to, std::vector<PendingOp> &ops) {
    Gene &G = genes[g];
    const int nt = G.aln.ntax;
    if (v < nt || virt_kind(g, v, to)) return 0;
    {                                                   // most calls ask for a message that is valid or already pending
        const int idx0 = (v - nt) * 3 + G.tree.slot(v, to);
        if (G.valid[idx0]) return 0;
        if (G.pend_level[idx0] >= 0) return G.pend_level[idx0];
    }
    // explicit stack (trees can be caterpillars of depth ~ntax)
    struct Frame { int v, to, k, stage, lv[2]; };
    std::vector<Frame> st;
    st.reserve(64);
    st.push_back({v, to, G.tree.slot(v, to), 0, {0, 0}});
    int ret = 0;
    while (!st.empty()) {
        Frame &f = st.back();
        const int idx = (f.v - nt) * 3 + f.k;
        if (f.stage == 0) {
            if (G.valid[idx]) { ret = 0; st.pop_back(); continue; }
            if (G.pend_level[idx] >= 0) { ret = G.pend_level[idx]; st.pop_back(); continue; }
        }
        int ch[2], ci = 0;
        for (int q = 0; q < 3; ++q) if (q != f.k) ch[ci++] = G.tree.nbr[f.v][q];
        if (f.stage >= 1) f.lv[f.stage - 1] = ret;
        if (f.stage < 2) {
            const int c = ch[f.stage];
            f.stage++;
            if (c < nt || virt_kind(g, c, f.v)) { ret = 0; continue; }   // tip / virtual (cherry, pitchfork) child: nothing to compute
            const int fv = f.v;
            st.push_back({c, fv, G.tree.slot(c, fv), 0, {0, 0}});
            continue;
        }
        const int lvl = std::max(f.lv[0], f.lv[1]) + 1;
        PendingOp op; op.gene = g; op.out_kind = SIDE_MSG; op.out_id = idx; op.level = lvl; ci = 0;
        for (int q = 0; q < 3; ++q) if (q != f.k) { op.child[ci] = msg(g, G.tree.nbr[f.v][q], f.v); op.t[ci] = G.tree.len[f.v][q]; ci++; }
        ops.push_back(op);
        G.pend_level[idx] = lvl;
        ret = lvl;
        st.pop_back();
    }
    return ret;
}

// ------------------------------------------------------------------------------------------
// requests
// ------------------------------------------------------------------------------------------
int Batch::evaluate(const std::vector<char> &active, double *lnl) {
    ++cnt_eval;
    std::vector<PendingOp> ops; std::vector<Tail> tails;
    for (int g = 0; g < (int)genes.size(); ++g) {
        if (!active.empty() && !active[g]) continue;
        Gene &G = genes[g];
        const int r = G.tree.nbr[0][0];
        need(g, r, 0, ops);
        tails.push_back({g, msg(g, 0, r), msg(g, r, 0), MODE_EVALUATE, G.tree.len[0][0], 0, 0, -1, 0, 0});
    }
    if (int rc = run(ops, tails)) return rc;
    for (auto &t : tails) lnl[t.gene] = res(t.gene)[0];
    for (auto &t : tails) det_record(det_id, genes[t.gene], 'E', 0, 0, lnl[t.gene], genes[t.gene].alpha, 0);
    return 0;
}
int Batch::score(const std::vector<char> &active, double *lnl, bool stored) {
    for (int g = 0; g < (int)genes.size(); ++g) if (active.empty() || active[g]) invalidate_all(g);
    bool all = true;
    for (char a : active) all = all && a;
    if (all && !score_only_batch) {
        if (plan.valid && plan.epoch == topo_epoch && plan.stored == stored) return replay_plan(lnl);
        record_plan = true; record_stored = stored;
    }
    const int rc = evaluate(active, lnl);
    record_plan = false; record_stored = false;
    return rc;
}
int Batch::site_lnl(int g, double *out) {
    Gene &G = genes[g];
    if ((int)G.aln.site2pat.size() != G.aln.nsites) return ctx->fail(-1, "per-site lnL is not available for device-gathered replicates");
    std::vector<char> act(genes.size(), 0); act[g] = 1;
    std::vector<double> l(genes.size());
    if (int rc = evaluate(act, l.data())) return rc;
    std::vector<double> pat(G.aln.mpad);
    HIPCHK(hipMemcpy(pat.data(), G.d_patlnl[0], sizeof(double) * G.aln.mpad, hipMemcpyDeviceToHost));
    for (int s = 0; s < G.aln.nsites; ++s) out[s] = pat[G.aln.site2pat[s]];
    return 0;
}
int Batch::root_derivs(double *lnl, double *d1, double *d2) {
    std::vector<PendingOp> ops; std::vector<Tail> tails;
    for (int g = 0; g < (int)genes.size(); ++g) {
        Gene &G = genes[g];
        const int r = G.tree.nbr[0][0];
        need(g, r, 0, ops);
        tails.push_back({g, msg(g, 0, r), msg(g, r, 0), MODE_SUMTABLE, G.tree.len[0][0], 0});
    }
    if (int rc = run(ops, tails)) return rc;
    for (int g = 0; g < (int)genes.size(); ++g) { lnl[g] = res(g)[1]; d1[g] = res(g)[2]; d2[g] = res(g)[3]; }
    return 0;
}

// one Gauss-Seidel pass over the dirty branches (DFS from taxon 0, oracle order: eng_smooth_rec)
int Batch::smooth_pass(const std::vector<char> &active, std::vector<double> &maxdelta, double thr) {
    const int n = (int)genes.size();
    maxdelta.assign(n, 0.0);
    struct SafeOff { bool &f; ~SafeOff() { f = false; } } safe_off{safe_now};     // whichever way the pass is left
    double hp_t = now_ms();
    // per-gene DFS edge order, restricted to dirty branches
    // (scratch kept between passes: this set-up runs while the device is idle)
    std::vector<std::vector<std::pair<int, int>>> &order = pass_order;
    std::vector<std::vector<uint8_t>> &next = pass_next;
    if ((int)order.size() != n) { order.assign(n, {}); next.assign(n, {}); }
    size_t maxlen = 0;
    struct F { int v, from, k; };
    std::vector<F> st; st.reserve(256);
    for (int g = 0; g < n; ++g) {
        order[g].clear();
        if (!active[g]) { next[g].clear(); continue; }
        Gene &G = genes[g];
        const Tree &T = G.tree; const int nt = T.ntax;
        if (G.dirty.size() != (size_t)T.nnodes() * 3) G.mark_all();
        next[g].assign((size_t)T.nnodes() * 3, 0);
        // emulate the recursion: visit(v, from): for k: edge (v,w); if inner recurse
        // (edge list fixed up-front: topology does not change during a pass)
        st.clear(); st.push_back({0, -1, 0});
        while (!st.empty()) {
            F &f = st.back();
            if (f.k >= 3) { st.pop_back(); continue; }
            const int k = f.k, w = T.nbr[f.v][k]; f.k++;
            if (w < 0 || w == f.from) continue;
            if (G.dirty[f.v * 3 + k]) order[g].push_back({f.v, w});
            if (w >= nt) { const int fv = f.v; st.push_back({w, fv, 0}); }
        }
        maxlen = std::max(maxlen, order[g].size());
    }
    ++cnt_passes;
    host_phase_ms[HP_PASS_SETUP] += now_ms() - hp_t; hp_t = now_ms();
    // The whole pass is enqueued without a host round trip: a branch optimised at step i has its new length in
    // Gene::d_len (written by k_newton), and every later transition-matrix request across that branch reads it from
    // there (PmatReq::tp).  The host learns the new lengths after ONE synchronisation at the end of the pass.
    size_t nres = 0; for (int g = 0; g < n; ++g) nres += order[g].size();
    struct Done { int gene, v, w; double old; size_t idx; };
    std::vector<Done> done; done.reserve(nres);
    // attempt 1 re-runs the WHOLE pass through the no-exchange Newton form when k_newton's exchange gave up somewhere in the
    // chained attempt 0: the host's branch lengths are still those of the pass start (new lengths live on the device until the
    // pass is accepted), the dirty flags are untouched, and CLVs computed from unaccepted lengths are invalidated -- so the
    // second attempt computes exactly what an untroubled pass computes
    for (int attempt = 0; attempt < 2; ++attempt) {
    done.clear();
    if (int rc = chain_begin(nres)) return rc;
    for (size_t step = 0; step < maxlen; ++step) {
        ++cnt_smooth;
        const size_t first = done.size();
        std::vector<PendingOp> ops; std::vector<Tail> tails;
        for (int g = 0; g < n; ++g) {
            if (!active[g] || step >= order[g].size()) continue;
            auto [v, w] = order[g][step];
            Gene &G = genes[g];
            need(g, v, w, ops); need(g, w, v, ops);
            Tail t{g, msg(g, v, w), msg(g, w, v), MODE_SUMTABLE, G.tree.len[v][G.tree.slot(v, w)], 32};
            t.result_dev = d_chain + 4 * done.size();
            t.t_dev0 = G.d_len + (size_t)v * 3 + G.tree.slot(v, w); t.t_dev1 = G.d_len + (size_t)w * 3 + G.tree.slot(w, v);
            done.push_back({g, v, w, t.t0, done.size()});
            tails.push_back(t);
        }
        if (tails.empty()) continue;
        if (int rc = run(ops, tails)) { chain_sync(); chain = false; return rc; }
        // the new length is on the device only: later requests across (v,w) take it from d_len
        for (size_t i = first; i < done.size(); ++i) {
            Gene &G = genes[done[i].gene]; const int v = done[i].v, w = done[i].w;
            G.len_pending[(size_t)v * 3 + G.tree.slot(v, w)] = 1; G.len_pending[(size_t)w * 3 + G.tree.slot(w, v)] = 1;
            branch_changed(done[i].gene, v, w);
        }
    }
    host_phase_ms[HP_PASS_STEPS] += now_ms() - hp_t;
    const double t0 = now_ms();
    if (int rc = chain_sync()) { chain = false; return rc; }
    ctx->stats[K_HOST_WAIT].launches++; ctx->stats[K_HOST_WAIT].ms += now_ms() - t0;
    host_phase_ms[HP_PASS_SYNC] += now_ms() - t0; hp_t = now_ms();
    chain = false;
    bool gave_up = false;
    for (auto &d : done) gave_up = gave_up || !std::isfinite(h_chain[4 * d.idx + 1]);
    if (gave_up) {
        if (attempt == 1 || safe_now) return ctx->fail(-5, "k_newton: non-finite branch likelihood (also from the no-exchange form)");
        newton_gave_up(); ctx->newton_reissued += (long long)done.size();
        if (int rc = clear_abort()) return rc;
        for (int g = 0; g < n; ++g) if (active[g]) { std::fill(genes[g].len_pending.begin(), genes[g].len_pending.end(), 0); invalidate_all(g); }
        safe_now = true;
        continue;
    }
    for (auto &d : done) {
        Gene &G = genes[d.gene];
        const double nl = h_chain[4 * d.idx], dl = std::fabs(nl - d.old);
        det_record(det_id, G, 'S', d.v, d.w, d.old, nl, h_chain[4 * d.idx + 1]);
        maxdelta[d.gene] = std::max(maxdelta[d.gene], dl);
        G.tree.set_len(d.v, d.w, nl);
        if (dl > thr) { std::swap(G.dirty, next[d.gene]); G.mark_node(d.v); G.mark_node(d.w); std::swap(G.dirty, next[d.gene]); }
    }
    for (auto &G : genes) std::fill(G.len_pending.begin(), G.len_pending.end(), 0);
    break;
    }   // attempts
    safe_now = false;
    for (int g = 0; g < n; ++g) if (active[g]) genes[g].dirty.swap(next[g]);
    host_phase_ms[HP_PASS_POST] += now_ms() - hp_t;
    return 0;
}

// FastTree's `-gamma` likelihood (FastTreeRunner.java:67-70 always passes it): the tree's per-pattern likelihoods at 20
// fixed rates, re-weighted by a discretised Gamma(alpha) whose mean is 1/mult; alpha and mult are fitted by alternating
// one-dimensional Brent searches on log alpha / log mult in [0.01, 10] (tolerance 1e-3, <= 10 rounds, stop when a round
// gains < 1e-3), the spec of oracle/pml_oracle.c po_gamma20.  Reported: Gamma20 lnL, alpha, rescale = 1/mult (FastTree
// prints the tree with lengths x rescale).  Device work: five full traversals writing the table, then one tiny k_g20
// launch per objective evaluation for all genes together.
int Batch::gamma20(std::vector<double> &lnl20, std::vector<double> &alpha20, std::vector<double> &rescale20) {
    const int n = (int)genes.size();
    HIPCHK(hipSetDevice(ctx->device));
    double rates[G20_RATES]; g20_rates(rates);
    std::vector<size_t> off(n); size_t bytes = 0;
    for (int g = 0; g < n; ++g) { off[g] = bytes; bytes += align_up((size_t)genes[g].aln.mpad * (G20_RATES * 8 + (G20_RATES / 4) * 4), 256); }
    if (int rc = ensure_tailpool(bytes)) return rc;
    auto table = [&](int g) { return reinterpret_cast<double *>(d_tailpool + off[g]); };
    auto counts = [&](int g) { return reinterpret_cast<int *>(d_tailpool + off[g] + (size_t)genes[g].aln.mpad * G20_RATES * 8); };
    // the genes carry FastTree's fixed rates only inside the loop below: whatever way it is left, they get their Gamma4 rates back
    struct RatesBack { Batch *b; ~RatesBack() { for (int g = 0; g < (int)b->genes.size(); ++g) b->set_alpha(g, b->genes[g].alpha); } };
    for (int j = 0; j < G20_RATES / 4; ++j) {
        RatesBack back{this};
        std::vector<PendingOp> ops; std::vector<Tail> tails;
        for (int g = 0; g < n; ++g) {
            Gene &G = genes[g];
            for (int c = 0; c < 4; ++c) G.rates[c] = rates[4 * j + c];
            ++G.rates_epoch; invalidate_all(g);
            const int r = G.tree.nbr[0][0];
            need(g, r, 0, ops);
            Tail t{g, msg(g, 0, r), msg(g, r, 0), MODE_EVALUATE_CAT, G.tree.len[0][0], 0, 0, -1, 0, 0};
            t.patlnl_dev = table(g) + (size_t)4 * j * G.aln.mpad; t.scl_dev = counts(g) + (size_t)j * G.aln.mpad;
            tails.push_back(t);
        }
        if (int rc = run(ops, tails)) return rc;
    }
    if (int rc = ensure_results((size_t)n)) return rc;
    if (int rc = ensure_stage((size_t)n * sizeof(G20Req))) return rc;
    std::vector<double> la(n, 0.0), lm(n, 0.0), f(n, 0.0);               // log alpha, log mult, -lnL
    auto objective = [&](const std::vector<char> &act) -> int {
        G20Req *h = (G20Req *)h_stage; int k = 0;
        std::vector<int> who;
        for (int g = 0; g < n; ++g) {
            if (!act[g]) continue;
            G20Req &r = h[k++];
            r.table = table(g); r.cnt = counts(g); r.weight = genes[g].d_weight; r.out = d_chain + 4 * g; r.patlnl = nullptr;
            r.mpad = genes[g].aln.mpad; r.pad = 0;
            g20_weights(std::exp(la[g]), std::exp(lm[g]), r.w);
            who.push_back(g);
        }
        if (!k) return 0;
        HIPCHK(hipMemcpyAsync(d_stage, h_stage, (size_t)k * sizeof(G20Req), hipMemcpyHostToDevice, ctx->stream));
        launch_g20((const G20Req *)d_stage, k, ctx->stream);
        results_used = (size_t)n;
        if (int rc = fetch_results(true)) return rc;
        { if (int rc_ = ctx->sync(ctx->stream)) return rc_; }
        HIPCHK(hipGetLastError());
        for (int g : who) { f[g] = -h_chain[4 * g]; if (!std::isfinite(f[g])) return ctx->fail(-5, "device returned a non-finite Gamma20 likelihood"); }
        return 0;
    };
    std::vector<char> all(n, 1), active(n, 1);
    if (int rc = objective(all)) return rc;
    const double LO = std::log(0.01), HI = std::log(10.0), TOL = 1e-3;
    for (int round = 0; round < 10; ++round) {
        bool any = false; for (char a : active) any |= a;
        if (!any) break;
        const std::vector<double> start(f);
        for (int which = 0; which < 2; ++which) {                          // 0: alpha, 1: mult
            std::vector<double> &x = which ? lm : la;
            std::vector<Brent> br(n);
            std::vector<char> act(active);
            for (int g = 0; g < n; ++g) if (act[g]) br[g].start(LO, HI, x[g], f[g], TOL);
            for (;;) {
                bool moved = false;
                for (int g = 0; g < n; ++g) { if (!act[g]) continue; if (br[g].propose()) { x[g] = br[g].u; moved = true; } else act[g] = 0; }
                if (!moved) break;
                if (int rc = objective(act)) return rc;
                for (int g = 0; g < n; ++g) if (act[g]) br[g].update(f[g]);
            }
            for (int g = 0; g < n; ++g) if (active[g]) { x[g] = br[g].x; f[g] = br[g].fx; }
        }
        for (int g = 0; g < n; ++g) if (active[g] && !(f[g] < start[g] - 1e-3)) active[g] = 0;
    }
    lnl20.resize(n); alpha20.resize(n); rescale20.resize(n);
    for (int g = 0; g < n; ++g) { lnl20[g] = -f[g]; alpha20[g] = std::exp(la[g]); rescale20[g] = std::exp(-lm[g]); }
    return 0;
}

// Brent on log(alpha) per gene, all genes in lock step (one full-traversal evaluation of every active gene per
// iteration).  Control flow = the oracle's eng_opt_alpha: +-ln 4 window around the current value, doubled and
// continued when the minimum ends at a window edge that is not a global limit.
int Batch::opt_alpha(const std::vector<char> &active, double *lnl, double tol) {
    const int n = (int)genes.size();
    const double LMIN = std::log(ALPHA_MIN), LMAX = std::log(ALPHA_MAX);
    std::vector<Brent> br(n);
    std::vector<char> act(active);
    std::vector<double> f(n), W(n, std::log(4.0)), lo(n), hi(n);
    std::vector<int> win(n, 0);
    if (int rc = score(act, f.data())) return rc;
    auto open_window = [&](int g, double x, double fx) {
        lo[g] = std::max(LMIN, x - W[g]); hi[g] = std::min(LMAX, x + W[g]);
        br[g].start(lo[g], hi[g], x, fx, tol);
    };
    for (int g = 0; g < n; ++g) if (act[g]) open_window(g, std::log(genes[g].alpha), -f[g]);
    for (;;) {
        bool any = false;
        const double hp_a = now_ms();
        for (int g = 0; g < n; ++g) {
            if (!act[g]) continue;
            for (;;) {
                if (br[g].propose()) { set_alpha(g, std::exp(br[g].u)); any = true; break; }
                const double x = br[g].x, edge = 4 * tol;
                if (++win[g] < 8 && ((x - lo[g] < edge && lo[g] > LMIN) || (hi[g] - x < edge && hi[g] < LMAX))) { W[g] *= 2; open_window(g, x, br[g].fx); continue; }
                act[g] = 0; break;
            }
        }
        host_phase_ms[HP_ALPHA_HOST] += now_ms() - hp_a;
        if (!any) break;
        if (int rc = score(act, f.data())) return rc;
        for (int g = 0; g < n; ++g) if (act[g]) br[g].update(-f[g]);
    }
    for (int g = 0; g < n; ++g) if (active[g]) { set_alpha(g, std::exp(br[g].x)); lnl[g] = -br[g].fx; }
    return 0;
}

// PROTGAMMAGTR: one sweep over the 189 free exchangeabilities (the last of the 190 stays 1: a common factor of all rates
// cancels in the normalisation to one substitution per site) of every active GTR gene.  Rate k of all genes is optimised
// in lock step by Brent on log(rate), the window logic of opt_alpha (+-ln 4 around the current value, doubled and continued
// while the minimum sits on a window edge that is not a global bound).  One trial = k_model for the active genes with rate k
// patched (nothing is uploaded but the requests) -> k_eigfrags -> the scoring step; the host reads the lnL and nothing else.
// The accepted value is written to the device copy of the gene's exchangeabilities before the next rate starts.
int Batch::opt_rates(const std::vector<char> &active, double *lnl, double tol) {
    const int n = (int)genes.size();
    std::vector<char> gtr(n, 0);
    std::vector<int> all;
    for (int g = 0; g < n; ++g) if (active[g] && genes[g].model_code == PM_GTR) { gtr[g] = 1; all.push_back(g); }
    if (all.empty()) return 0;
    const double t0 = now_ms(); const long trials0 = cnt_rate_trials;
    const double LMIN = std::log(RATE_MIN), LMAX = std::log(RATE_MAX);
    std::vector<double> f(n), fu(n), vals; std::vector<int> gs;
    if (int rc = score(gtr, fu.data())) return rc;
    for (int g : all) f[g] = -fu[g];
    std::vector<Brent> br(n);
    std::vector<double> W(n), lo(n), hi(n);
    std::vector<int> win(n);
    for (int k = 0; k < NEXCH - 1; ++k) {
        std::vector<char> act(gtr);
        auto open_window = [&](int g, double x, double fx) {
            lo[g] = std::max(LMIN, x - W[g]); hi[g] = std::min(LMAX, x + W[g]);
            br[g].start(lo[g], hi[g], x, fx, tol);
        };
        for (int g : all) {
            W[g] = std::log(4.0); win[g] = 0;
            open_window(g, std::min(LMAX, std::max(LMIN, std::log(h_gexch[(size_t)g * NEXCH + k]))), f[g]);
        }
        for (;;) {
            gs.clear(); vals.clear();
            for (int g : all) {
                if (!act[g]) continue;
                for (;;) {
                    if (br[g].propose()) { gs.push_back(g); vals.push_back(std::exp(br[g].u)); break; }
                    const double x = br[g].x, edge = 4 * tol;
                    if (++win[g] < 8 && ((x - lo[g] < edge && lo[g] > LMIN) || (hi[g] - x < edge && hi[g] < LMAX))) { W[g] *= 2; open_window(g, x, br[g].fx); continue; }
                    act[g] = 0; break;
                }
            }
            if (gs.empty()) break;
            if (int rc = build_models(gs, k, vals.data())) return rc;
            cnt_rate_trials += (long)gs.size();
            if (int rc = score(act, fu.data())) return rc;
            for (int g : gs) br[g].update(-fu[g]);
        }
        for (int g : all) { h_gexch[(size_t)g * NEXCH + k] = std::exp(br[g].x); f[g] = br[g].fx; }
        HIPCHK(hipMemcpyAsync(d_gexch, h_gexch, (size_t)n * NEXCH * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    }
    // the models of the accepted rates (a gene's last trial is not its best one)
    if (int rc = build_models(all, -1, nullptr)) return rc;
    if (int rc = ctx->sync(ctx->stream)) return rc;
    HIPCHK(hipGetLastError());
    for (int g : all) { invalidate_all(g); lnl[g] = -f[g]; }
    if (std::getenv("PML_TRACE")) fprintf(stderr, "[pml] rates sweep: %d genes, %ld model builds + scoring steps, %.1f ms\n", (int)all.size(), cnt_rate_trials - trials0, now_ms() - t0);
    return 0;
}

int Batch::optimize(bool opt_alpha_flag, double eps, double *lnl, const std::vector<char> *mask) {
    const int n = (int)genes.size();
    std::vector<char> active(n, 1);
    if (mask) active = *mask;
    for (int g = 0; g < n; ++g) {
        if (!active[g]) continue;
        Tree &T = genes[g].tree;
        T.map_len([](double x) { return x < TMIN ? TMIN : x; });
        invalidate_all(g);
    }
    const std::vector<char> initial(active);
    std::vector<double> cur(n), nl(n), md;
    if (int rc = evaluate(active, cur.data())) return rc;
    // precision follows eps (oracle: po_engine_optimize): passes stop when max |dt| < thr =
    // clamp(eps/100, 1e-6, 1e-3), Newton stops at thr/100; <= 8 passes per round for eps >= 0.05,
    // <= 16 otherwise; every round starts with all branches dirty
    const int maxpass = eps >= 0.05 ? 8 : 16;
    const double thr = std::min(1e-3, std::max(1e-6, eps * 0.01)), save_tol = newton_tol;
    newton_tol = thr * 0.01;
    struct Restore { double &r; double v; ~Restore() { r = v; } } restore{newton_tol, save_tol};
    for (int round = 0; round < 100; ++round) {
        bool any = false; for (char a : active) any |= a;
        if (!any) break;
        std::vector<char> sm(active);
        for (int g = 0; g < n; ++g) if (sm[g]) genes[g].mark_all();
        // geometric pass budget 1, 2, 4, ... maxpass: while alpha is still moving a lot, branch lengths
        // are not polished to thr (they shift again with the next alpha)
        const int budget = opt_alpha_flag ? std::min(maxpass, 1 << std::min(round, 5)) : maxpass;
        for (int pass = 0; pass < budget; ++pass) {
            bool anys = false; for (char a : sm) anys |= a;
            if (!anys) break;
            if (int rc = smooth_pass(sm, md, thr)) return rc;
            for (int g = 0; g < n; ++g) if (sm[g] && md[g] < thr) sm[g] = 0;
        }
        // a round of a GTR gene: branch smoothing, all rates, alpha (cyclic: the order the rounds repeat is what matters)
        if (rates_on && d_gexch) { if (int rc = opt_rates(active, nl.data(), eps >= 0.05 ? 1e-2 : 1e-3)) return rc; }
        if (opt_alpha_flag) { if (int rc = opt_alpha(active, nl.data(), eps >= 0.05 ? 1e-2 : 1e-4)) return rc; }
        else { if (int rc = evaluate(active, nl.data())) return rc; }
        for (int g = 0; g < n; ++g) {
            if (!active[g]) continue;
            const double gain = nl[g] - cur[g]; cur[g] = nl[g];
            if (gain < eps) active[g] = 0;
        }
    }
    for (int g = 0; g < n; ++g) if (initial[g]) lnl[g] = cur[g];
    if (std::getenv("PML_TRACE")) fprintf(stderr, "[pml] optimize(eps %g): cumulative passes %ld smooth-steps %ld evals %ld\n", eps, cnt_passes, cnt_smooth, cnt_eval);
    return 0;
}

}  // namespace pml
