// boot.cpp -- the column bootstrap as a resident call (include/peprml.h pml_bootstrap2): `raxmlHPC -f a -x seed -N reps` and
// `-Y -N reps` on the concatenation of a gene set, the path PhylogenomicPipeline2.buildConcatenatedTree (:836-890) takes with
// bootstrapReps.  The genes are encoded once (GeneStore); every replicate is a re-weighted, compacted view of the resident patterns,
// built by the four kernels of boot.hip under the draw rule of boot.hpp, and the replicates are searched as device batches (ML:
// Batch::create_bootstrap + the NNI search from the NJ start; parsimony: parsimony_bootstrap).  No resampled text exists anywhere.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>

#include "../../include/peprml.h"
#include "api_types.hpp"
#include "boot_dev.hpp"

using namespace pml;

#define BCHK(expr)                                                                          \
    do { hipError_t e_ = (expr);                                                                   \
         if (e_ != hipSuccess) return ctx->fail(-4, std::string("bootstrap: ") + hipGetErrorString(e_)); } while (0)

namespace {
// HIP-event time of one launch in profile mode: start() before it, stop() after it, add() once the stream has been synchronised
struct LaunchTimer {
    Ctx *ctx; int k; hipEvent_t a = nullptr, b = nullptr;
    LaunchTimer(Ctx *c, int kind) : ctx(c), k(kind) { ctx->boot_launches[k]++; if (ctx->profile && (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess)) { drop(); } }
    void start() { if (a) hipEventRecord(a, ctx->stream); }
    void stop() { if (b) hipEventRecord(b, ctx->stream); }
    void add() { float ms = 0; if (a && b && hipEventElapsedTime(&ms, a, b) == hipSuccess) ctx->boot_ms[k] += ms; drop(); }
    void drop() { if (a) hipEventDestroy(a); if (b) hipEventDestroy(b); a = b = nullptr; }
    ~LaunchTimer() { drop(); }
};
char *dup_cstr(const std::string &s) { char *p = (char *)std::malloc(s.size() + 1); if (p) std::memcpy(p, s.c_str(), s.size() + 1); return p; }
template <class T> T *dup_vec(const std::vector<T> &v) {
    T *p = (T *)std::malloc(std::max<size_t>(v.size(), 1) * sizeof(T));
    if (p && !v.empty()) std::memcpy(p, v.data(), v.size() * sizeof(T));
    return p;
}
}  // namespace

namespace pml {

int BootSet::create(Ctx *c, const GeneStore &store, const std::vector<int> &sel) {
    ctx = c;
    if (sel.empty()) return ctx->fail(-1, "bootstrap: no genes selected");
    std::vector<long long> ns;
    for (int g : sel) {
        if (g < 0 || g >= (int)store.items.size()) return ctx->fail(-1, "gene index out of range");
        names.insert(names.end(), store.items[g].aln.names.begin(), store.items[g].aln.names.end());
        ns.push_back(store.items[g].aln.nsites);
    }
    std::sort(names.begin(), names.end()); names.erase(std::unique(names.begin(), names.end()), names.end());
    const int nt = (int)names.size();
    if (nt < 3) return ctx->fail(-1, "bootstrap: fewer than 3 taxa in the union of the genes");
    std::string err;
    L = boot_total_columns((int)ns.size(), ns.data(), err);
    if (L < 0) return ctx->fail(-1, "bootstrap: " + err);
    nseg = (int)sel.size();
    std::vector<BootSeg> segs((size_t)nseg);
    std::vector<int> rowmaps((size_t)nseg * nt, -1);
    col2pat.clear(); col2pat.reserve((size_t)L);
    P = 0;
    for (int i = 0; i < nseg; ++i) {
        const GeneStore::Item &it = store.items[sel[i]];
        segs[i] = BootSeg{it.d_codes, it.aln.mpad, P, it.aln.npat, 0};
        for (int t = 0; t < it.aln.ntax; ++t) rowmaps[(size_t)i * nt + (size_t)(std::lower_bound(names.begin(), names.end(), it.aln.names[t]) - names.begin())] = t;
        for (int s = 0; s < it.aln.nsites; ++s) col2pat.push_back(P + it.aln.site2pat[s]);
        P += it.aln.npat;
    }
    const size_t o_seg = align_up(col2pat.size() * sizeof(int), 256), o_map = o_seg + align_up(segs.size() * sizeof(BootSeg), 256),
                 total = o_map + rowmaps.size() * sizeof(int);
    BCHK(hipSetDevice(ctx->device));
    BCHK(hipMalloc((void **)&d_buf, total));
    BCHK(hipMemcpyAsync(d_buf, col2pat.data(), col2pat.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    BCHK(hipMemcpyAsync(d_buf + o_seg, segs.data(), segs.size() * sizeof(BootSeg), hipMemcpyHostToDevice, ctx->stream));
    BCHK(hipMemcpyAsync(d_buf + o_map, rowmaps.data(), rowmaps.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    if (int rc = ctx->sync(ctx->stream)) return rc;              // the host vectors go out of scope
    sp = BootSpace{(const int *)d_buf, (const BootSeg *)(d_buf + o_seg), (const int *)(d_buf + o_map), (unsigned)L, P, nseg, nt};
    return 0;
}

int BootReps::count_and_index(Ctx *c, const BootSet &s, int begin, int end, unsigned long long seed) {
    ctx = c; set = &s; n = end - begin;
    if (n <= 0 || begin < 0) return ctx->fail(-1, "bootstrap: empty range of replicates");
    if (n > BOOT_MAX_REPS) return ctx->fail(-1, "bootstrap: a sub-batch holds at most " + std::to_string(BOOT_MAX_REPS) + " replicates");
    const size_t P = (size_t)s.P, o_count = align_up((size_t)n * sizeof(BootRep), 256), o_idx = o_count + align_up((size_t)n * P * 4, 256),
                 o_npat = o_idx + align_up((size_t)n * P * 4, 256), total = o_npat + (size_t)n * sizeof(int);
    BCHK(hipSetDevice(ctx->device));
    BCHK(hipMalloc((void **)&d_buf, total));
    d_reps = (BootRep *)d_buf;
    h.assign((size_t)n, BootRep{});
    for (int r = 0; r < n; ++r) {
        h[r].key = boot_key(seed, (uint32_t)(begin + r));
        h[r].count = (unsigned *)(d_buf + o_count) + (size_t)r * P;
        h[r].idx = (int *)(d_buf + o_idx) + (size_t)r * P;
        h[r].npat_dev = (int *)(d_buf + o_npat) + r;
    }
    BCHK(hipMemcpyAsync(d_reps, h.data(), (size_t)n * sizeof(BootRep), hipMemcpyHostToDevice, ctx->stream));
    BCHK(hipMemsetAsync(d_buf + o_count, 0, (size_t)n * P * 4, ctx->stream));
    const char *e = std::getenv("PML_BOOT_GLOBAL_HIST");
    LaunchTimer tc(ctx, 0), ti(ctx, 1);
    tc.start(); launch_boot_count(s.sp, d_reps, n, e && *e && *e != '0', ctx->stream); tc.stop();
    ti.start(); launch_boot_index(s.sp, d_reps, n, ctx->stream); ti.stop();
    BCHK(hipGetLastError());
    npat.assign((size_t)n, 0);
    BCHK(hipMemcpyAsync(npat.data(), d_buf + o_npat, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    if (int rc = ctx->sync(ctx->stream)) return rc;
    tc.add(); ti.add();
    for (int r = 0; r < n; ++r) {
        if (npat[r] < 1 || npat[r] > s.P) return ctx->fail(-4, "bootstrap: the compaction of replicate " + std::to_string(begin + r) + " is out of range");
        h[r].npat = npat[r];
    }
    return 0;
}

int BootReps::gather(int form) {
    int max_mpad = 0;
    for (auto &r : h) { if (!r.dst || !r.dst_w || r.mpad < r.npat) return ctx->fail(-1, "bootstrap: a replicate has no destination"); max_mpad = std::max(max_mpad, r.mpad); }
    BCHK(hipMemcpyAsync(d_reps, h.data(), (size_t)n * sizeof(BootRep), hipMemcpyHostToDevice, ctx->stream));
    LaunchTimer tg(ctx, 2);
    tg.start(); launch_boot_gather(set->sp, d_reps, n, max_mpad, form, ctx->stream); tg.stop();
    BCHK(hipGetLastError());
    if (int rc = ctx->sync(ctx->stream)) return rc;
    tg.add();
    return 0;
}

int BootReps::pairs(std::vector<std::vector<int64_t>> &cmp, std::vector<std::vector<int64_t>> &diff) {
    const size_t nn = (size_t)set->sp.ntax * set->sp.ntax;
    BCHK(hipMalloc((void **)&d_pairs, (size_t)n * 2 * nn * sizeof(long long)));
    BCHK(hipMemsetAsync(d_pairs, 0, (size_t)n * 2 * nn * sizeof(long long), ctx->stream));
    for (int r = 0; r < n; ++r) { h[r].cmp = d_pairs + (size_t)r * 2 * nn; h[r].diff = h[r].cmp + nn; }
    BCHK(hipMemcpyAsync(d_reps, h.data(), (size_t)n * sizeof(BootRep), hipMemcpyHostToDevice, ctx->stream));
    LaunchTimer tp(ctx, 3);
    tp.start(); launch_boot_pairs(set->sp, d_reps, n, ctx->stream); tp.stop();
    BCHK(hipGetLastError());
    std::vector<long long> flat((size_t)n * 2 * nn);
    BCHK(hipMemcpyAsync(flat.data(), d_pairs, flat.size() * sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
    if (int rc = ctx->sync(ctx->stream)) return rc;
    tp.add();
    cmp.assign((size_t)n, {}); diff.assign((size_t)n, {});
    for (int r = 0; r < n; ++r) {
        cmp[r].assign(flat.begin() + (size_t)r * 2 * nn, flat.begin() + (size_t)r * 2 * nn + nn);
        diff[r].assign(flat.begin() + (size_t)r * 2 * nn + nn, flat.begin() + (size_t)(r + 1) * 2 * nn);
    }
    return 0;
}

int BootReps::read_idx(int r, std::vector<int> &idx) {
    idx.assign((size_t)npat[r], 0);
    BCHK(hipMemcpy(idx.data(), h[r].idx, idx.size() * sizeof(int), hipMemcpyDeviceToHost));
    return 0;
}

int Batch::create_bootstrap(Ctx *c, const GeneStore &store, const std::vector<int> &sel, int reps_begin, int reps_end, unsigned long long seed,
                            int pm, int nc, double alpha, const BootSet *set, BootDebug *dbg) {
    ctx = c; pi_mode = pm; ncat = nc; score_only_batch = false;
    virtual_cherries = std::getenv("PML_NO_CHERRY") == nullptr;
    virtual_pitch = virtual_cherries && std::getenv("PML_NO_PITCH") == nullptr;
    if (int rc = ctx->ensure_model(pm)) return rc;                 // also refuses an unknown code
    const bool per_gene = model_per_gene(pm);
    if (!per_gene) { d_shared = ctx->shared_of(pm)->d_model; d_shared_eig = ctx->shared_of(pm)->d_eigfrags; }
    BCHK(hipSetDevice(ctx->device));
    const double t0 = now_ms();
    BootSet own;
    if (!set) { if (int rc = own.create(ctx, store, sel)) return rc; set = &own; }
    BootReps br;
    if (int rc = br.count_and_index(ctx, *set, reps_begin, reps_end, seed)) return rc;
    const int n = br.n, nt = (int)set->names.size();
    genes.resize(n);
    for (int r = 0; r < n; ++r) {
        Gene &G = genes[r]; EncodedAlignment &A = G.aln;
        G.model_code = pm;
        A.ntax = nt; A.names = set->names; A.nsites = (int)set->L; A.npat = br.npat[r]; A.mpad = (A.npat + 31) / 32 * 32;
    }
    if (int rc = layout(alpha, false)) return rc;
    for (int r = 0; r < n; ++r) { br.h[r].dst = genes[r].d_codes; br.h[r].dst_w = genes[r].d_weight; br.h[r].mpad = genes[r].aln.mpad; }
    if (int rc = br.gather(BOOT_FORM_CODES)) return rc;            // writes the padding too: gap code, weight 0
    std::vector<std::vector<int64_t>> cmp, diff;
    if (int rc = br.pairs(cmp, diff)) return rc;
    for (int r = 0; r < n; ++r) { genes[r].tree = nj_from_counts(nt, cmp[r], diff[r]); genes[r].mark_all(); }
    ctx->boot_build_ms += now_ms() - t0;
    if (dbg) { if (int rc = br.read_idx(0, dbg->idx)) return rc; dbg->cmp = cmp[0]; dbg->diff = diff[0]; }
    if (!per_gene) return 0;
    // a model per replicate, as create_replicates builds one: the frequencies come from the replicate's matrix and weights
    if (int rc = count_replicate_freqs()) return rc;
    return build_gene_models();
}

}  // namespace pml

// ------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------
namespace {
// what is refused before a gene is encoded: the union's size and the concatenation's length, from the arguments alone
int check_genes(pml_ctx *ctx, int ngenes, const pml_alignment *genes, const std::vector<int> &sel) {
    // every gene is encoded into the store, selected or not
    for (int g = 0; g < ngenes; ++g) if (!genes[g].names || !genes[g].rows || genes[g].ntax <= 0) return ctx->c.fail(PML_EINVAL, "bad alignment");
    std::set<std::string> uni; std::vector<long long> ns;
    for (int g : sel) {
        if (g < 0 || g >= ngenes) return ctx->c.fail(PML_EINVAL, "gene index out of range");
        const pml_alignment &A = genes[g];
        if (!A.names || !A.rows || A.ntax <= 0 || A.nsites < 0) return ctx->c.fail(PML_EINVAL, "bad alignment");
        for (int i = 0; i < A.ntax; ++i) { if (!A.names[i]) return ctx->c.fail(PML_EINVAL, "bad alignment"); uni.insert(A.names[i]); }
        ns.push_back(A.nsites);
    }
    if (uni.size() < 3) return ctx->c.fail(PML_EINVAL, "bootstrap: fewer than 3 taxa in the union of the genes");
    std::string err;
    if (boot_total_columns((int)ns.size(), ns.data(), err) < 0) return ctx->c.fail(PML_EINVAL, "bootstrap: " + err);
    return PML_OK;
}
}  // namespace

extern "C" int pml_bootstrap2(pml_ctx *ctx, int ngenes, const pml_alignment *genes, const pml_model *model, const pml_bootstrap_opts2 *opts,
                              pml_result *best_out, char **replicate_newicks_out, long long *mp_lengths_out) {
    if (!ctx || !genes || ngenes <= 0 || !best_out) return PML_EINVAL;
    pml_fpguard fpg;
    std::memset(best_out, 0, sizeof *best_out);
    if (replicate_newicks_out) *replicate_newicks_out = nullptr;
    const int reps = opts ? opts->reps : 100, method = opts ? opts->method : PML_TREE_ML;
    const unsigned long long seed = opts ? opts->seed : 0;
    const int spr_best = opts ? opts->spr_radius_best : 5, radius = opts ? opts->parsimony_radius : 20;
    const double eps = (opts && opts->epsilon > 0) ? opts->epsilon : 1e-3;
    const pml_model *rm = (opts && opts->replicate_model) ? opts->replicate_model : model;
    std::lock_guard<std::mutex> lk(ctx->c.mu);
    ctx->c.boot_last_lnl.clear();                                // a refused or failed call leaves none behind (pml_boot_replicate_lnls)
    // everything is refused here, before a gene is encoded or uploaded
    if (reps < 0) return ctx->c.fail(PML_EINVAL, "bootstrap: reps must not be negative");
    if (method != PML_TREE_ML && method != PML_TREE_PARSIMONY && method != PML_TREE_PARSIMONY_BL) return ctx->c.fail(PML_EINVAL, "bad method " + std::to_string(method));
    if (radius < 0) return ctx->c.fail(PML_EINVAL, "parsimony_radius must not be negative");
    const pml_model *used[2] = {method == PML_TREE_PARSIMONY ? nullptr : model, method == PML_TREE_ML ? rm : nullptr};
    for (const pml_model *m : used) {
        if (m && !ctx->c.valid_code(m->pi_mode)) return ctx->c.fail(PML_EINVAL, "bad pi_mode " + std::to_string(m->pi_mode));
        if (m && m->ncat != 1 && m->ncat != 4) return ctx->c.fail(PML_EINVAL, "ncat must be 1 or 4");
    }
    std::vector<int> all(ngenes); for (int i = 0; i < ngenes; ++i) all[i] = i;
    if (int rc = check_genes(ctx, ngenes, genes, all)) return rc;
    if (mp_lengths_out) for (int i = 0; i <= reps; ++i) mp_lengths_out[i] = -1;
    pml_drop_worker_caches(ctx);
    try {
        GeneStore store;
        struct Drop { GeneStore &s; ~Drop() { s.destroy(); } } drop{store};
        static_assert(sizeof(pml_alignment) == sizeof(pml_alignment_view), "alignment view layout");
        if (int rc = store.create(&ctx->c, ngenes, reinterpret_cast<const pml_alignment_view *>(genes))) return rc;
        BootSet set;
        if (int rc = set.create(&ctx->c, store, all)) return rc;
        const std::vector<std::string> &names = set.names;
        const int nt = (int)names.size();
        const int ncat = model ? model->ncat : 4, pm = model ? model->pi_mode : 0; const double alpha = model ? model->alpha : 1.0;
        const int rncat = rm ? rm->ncat : 4, rpm = rm ? rm->pi_mode : 0; const double ralpha = rm ? rm->alpha : 1.0;
        // ---- the best tree, on the replicate of all genes as pml_jackknife* builds its full tree ----
        Tree best; double lnl = 0, al = method == PML_TREE_PARSIMONY ? 0.0 : alpha;
        if (method == PML_TREE_ML) {
            Batch b; int rc = b.create_replicates(&ctx->c, store, {all}, pm, ncat, alpha);
            if (!rc) rc = b.search(true, spr_best, true, eps, &lnl);
            if (rc) { b.destroy(); return rc; }
            best = b.genes[0].tree; al = b.genes[0].alpha;
            b.destroy();
        } else {
            std::vector<Tree> pt; std::vector<std::vector<std::string>> pn; std::vector<long long> pl;
            if (int rc = parsimony_replicates(&ctx->c, store, {all}, {boot_parsimony_seed(seed, 0)}, radius, pt, pn, pl)) return rc;
            best = pt[0];
            if (mp_lengths_out) mp_lengths_out[0] = pl[0];
            if (method == PML_TREE_PARSIMONY_BL) {               // `-f e -t` on that topology: lengths from 0.1 and alpha, as pml_optimize runs them
                Batch b;
                struct DropB { Batch &b; ~DropB() { b.destroy(); } } dropb{b};
                if (int rc = b.create_replicates(&ctx->c, store, {all}, pm, ncat, alpha)) return rc;
                Gene &G = b.genes[0];
                std::string err;
                if (G.aln.names != names || !Tree::parse(best.newick(names, 6).c_str(), G.aln.names, G.tree, err))
                    return ctx->c.fail(PML_EINVAL, "parsimony tree does not fit the replicate of all genes: " + err);
                b.invalidate_all(0); G.mark_all(); ++b.topo_epoch;
                if (int rc = b.optimize(true, eps, &lnl)) return rc;
                best = G.tree; al = G.alpha;
            }
        }
        // ---- the replicates: sub-batches sized against free HBM by the largest a replicate can be (min(P, L) patterns) ----
        std::vector<Tree> trees((size_t)reps); std::string txt;
        if (reps > 0) {
            size_t free_b = 0, total_b = 0;
            if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = (size_t)1 << 40;
            size_t budget = (size_t)(0.85 * (double)(free_b + ctx->c.arena_cache_bytes));
            if (const char *e = std::getenv("PML_HBM_BUDGET_MB")) budget = (size_t)std::atoll(e) << 20;   // test hook
            const size_t pats = (size_t)std::min<long long>(set.P, set.L), n = (size_t)nt;
            size_t per_rep;
            if (method == PML_TREE_ML) {
                const size_t mp = (pats + 31) / 32 * 32, slots = 3 * (n - 2) + NSCRATCH + MAXTAIL;
                per_rep = slots * CLV_ROWS * ((mp + 127) / 128 * 128) * 8 + slots * mp * 4 + n * mp + 64 * mp + (1 << 16) + 2 * n * n * 8;
            } else {
                const size_t mp = std::max<size_t>(32, (pats + 31) / 32 * 32), groups = radius > 0 ? 64 : 1;
                per_rep = (n + 3 * (n - 2) + groups * (size_t)(radius + 2)) * mp * 4 + mp * 4;
                if (ctx->c.arena_cache) { hipFree(ctx->c.arena_cache); ctx->c.arena_cache = nullptr; ctx->c.arena_cache_bytes = 0; }   // the pools are allocations of their own
            }
            per_rep += boot_rep_bytes(set.P);
            // at most 65535 replicates a sub-batch: the kernels put the replicate on grid.y
            const int chunk = (int)std::max<size_t>(1, std::min<size_t>({(size_t)reps, budget / per_rep, (size_t)BOOT_MAX_REPS}));
            for (int begin = 0; begin < reps; begin += chunk) {
                const int end = std::min(reps, begin + chunk);
                if (method == PML_TREE_ML) {
                    Batch b; int rc = b.create_bootstrap(&ctx->c, store, all, begin, end, seed, rpm, rncat, ralpha, &set);
                    std::vector<double> l((size_t)(end - begin));
                    if (!rc) rc = b.search(true, 0, true, eps, l.data());
                    if (rc) { b.destroy(); return rc; }
                    for (int r = begin; r < end; ++r) { trees[r] = b.genes[r - begin].tree; txt += trees[r].newick(names, 6); txt += '\n'; ctx->c.boot_last_lnl.push_back(l[r - begin]); }
                    b.destroy();
                } else {
                    std::vector<Tree> pt; std::vector<long long> pl;
                    if (int rc = parsimony_bootstrap(&ctx->c, set, begin, end, seed, radius, pt, pl)) return rc;
                    for (int r = begin; r < end; ++r) {          // topology only, as pml_parsimony prints: nothing reads a replicate's lengths
                        trees[r] = pt[r - begin]; txt += trees[r].newick(names, -1); txt += '\n';
                        if (mp_lengths_out) mp_lengths_out[1 + r] = pl[r - begin];
                    }
                }
            }
        }
        const bool topo_only = method == PML_TREE_PARSIMONY;
        auto counts = support_counts(best, trees);
        if (reps > 0) for (auto &row : counts) for (int &c : row) if (c >= 0) c = (int)(0.5 + 100.0 * c / reps);   // percent, as RAxML_bipartitions
        best_out->lnl = lnl; best_out->alpha = al; best_out->tree_length = topo_only ? 0.0 : best.length();
        best_out->npatterns = set.P; best_out->nsites = (int)set.L;
        best_out->newick = dup_cstr(reps > 0 ? best.newick_labeled(names, topo_only ? -1 : 6, counts) : best.newick(names, topo_only ? -1 : 6));
        if (replicate_newicks_out) *replicate_newicks_out = dup_cstr(txt);
        if (!best_out->newick) return ctx->c.fail(PML_ENOMEM, "host allocation failed");
    } catch (const std::bad_alloc &) { return ctx->c.fail(PML_ENOMEM, "host allocation failed"); }
    catch (const std::exception &e) { return ctx->c.fail(PML_EINVAL, e.what()); }
    return PML_OK;
}

extern "C" int pml_debug_boot_replicate(pml_ctx *ctx, int ngenes, const pml_alignment *genes, int nsel, const int *sel, unsigned long long seed,
                                        int rep, int form, int *ntax_out, int *npat_out, int *mpad_out, int **idx_out, void **cells_out,
                                        void **weights_out, long long **cmp_out, long long **diff_out, char **names_out) {
    if (!ctx || !genes || ngenes <= 0 || !ntax_out || !npat_out || !mpad_out || !idx_out || !cells_out || !weights_out || !cmp_out || !diff_out ||
        !names_out || (sel && nsel <= 0)) return PML_EINVAL;
    *idx_out = nullptr; *cells_out = nullptr; *weights_out = nullptr; *cmp_out = nullptr; *diff_out = nullptr; *names_out = nullptr;
    std::lock_guard<std::mutex> lk(ctx->c.mu);
    if (rep < 0 || (form != 0 && form != 1)) return ctx->c.fail(PML_EINVAL, "bootstrap: rep must not be negative and form must be 0 or 1");
    std::vector<int> s;
    if (sel) s.assign(sel, sel + nsel); else { s.resize(ngenes); for (int i = 0; i < ngenes; ++i) s[i] = i; }
    if (int rc = check_genes(ctx, ngenes, genes, s)) return rc;
    pml_drop_worker_caches(ctx);
    try {
        GeneStore store;
        struct Drop { GeneStore &s; ~Drop() { s.destroy(); } } drop{store};
        if (int rc = store.create(&ctx->c, ngenes, reinterpret_cast<const pml_alignment_view *>(genes))) return rc;
        BootSet set;
        if (int rc = set.create(&ctx->c, store, s)) return rc;
        Batch b;
        struct DropB { Batch &b; ~DropB() { b.destroy(); } } dropb{b};
        BootDebug dbg;
        if (int rc = b.create_bootstrap(&ctx->c, store, s, rep, rep + 1, seed, 0, 4, 1.0, &set, &dbg)) return rc;
        const Gene &G = b.genes[0];
        const size_t nt = (size_t)G.aln.ntax;
        size_t mp = (size_t)G.aln.mpad;
        std::vector<unsigned char> cells; std::vector<unsigned char> wbytes;
        if (form == 0) {
            cells.resize(nt * mp); wbytes.resize(mp * sizeof(double));
            if (hipMemcpy(cells.data(), G.d_codes, nt * mp, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(wbytes.data(), G.d_weight, mp * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
                return ctx->c.fail(PML_EDEVICE, "read-back of the bootstrap replicate failed");
        } else {
            std::vector<unsigned> masks; std::vector<int> w; int np = 0, mpi = 0;
            if (int rc = boot_tips_readback(&ctx->c, set, rep, seed, &np, &mpi, masks, w)) return rc;
            if (np != G.aln.npat) return ctx->c.fail(PML_EDEVICE, "the two forms of the bootstrap replicate disagree on npat");
            mp = (size_t)mpi;
            cells.resize(masks.size() * sizeof(unsigned)); std::memcpy(cells.data(), masks.data(), cells.size());
            wbytes.resize(w.size() * sizeof(int)); std::memcpy(wbytes.data(), w.data(), wbytes.size());
        }
        std::string names; for (auto &n : G.aln.names) { names += n; names += '\n'; }
        *idx_out = dup_vec(dbg.idx); *cells_out = dup_vec(cells); *weights_out = dup_vec(wbytes);
        *cmp_out = (long long *)dup_vec(dbg.cmp); *diff_out = (long long *)dup_vec(dbg.diff); *names_out = dup_cstr(names);
        if (!*idx_out || !*cells_out || !*weights_out || !*cmp_out || !*diff_out || !*names_out) {
            for (void *p : {(void *)*idx_out, *cells_out, *weights_out, (void *)*cmp_out, (void *)*diff_out, (void *)*names_out}) std::free(p);
            *idx_out = nullptr; *cells_out = nullptr; *weights_out = nullptr; *cmp_out = nullptr; *diff_out = nullptr; *names_out = nullptr;
            return ctx->c.fail(PML_ENOMEM, "host allocation failed");
        }
        *ntax_out = (int)nt; *npat_out = G.aln.npat; *mpad_out = (int)mp;
    } catch (const std::bad_alloc &) { return ctx->c.fail(PML_ENOMEM, "host allocation failed"); }
    catch (const std::exception &e) { return ctx->c.fail(PML_EINVAL, e.what()); }
    return PML_OK;
}

extern "C" int pml_boot_replicate_lnls(pml_ctx *ctx, int n, double *lnl_out) {
    if (!ctx || n < 0 || (n > 0 && !lnl_out)) return PML_EINVAL;
    std::lock_guard<std::mutex> lk(ctx->c.mu);
    const int have = (int)ctx->c.boot_last_lnl.size();
    for (int i = 0; i < n && i < have; ++i) lnl_out[i] = ctx->c.boot_last_lnl[(size_t)i];
    return have;
}

extern "C" int pml_boot_stats(pml_ctx *ctx, long long *launches, double *kernel_ms, double *build_ms) {
    if (!ctx) return PML_EINVAL;
    std::lock_guard<std::mutex> lk(ctx->c.mu);
    for (int k = 0; k < 4; ++k) { if (launches) launches[k] = ctx->c.boot_launches[k]; if (kernel_ms) kernel_ms[k] = ctx->c.boot_ms[k]; }
    if (build_ms) *build_ms = ctx->c.boot_build_ms;
    return PML_OK;
}
