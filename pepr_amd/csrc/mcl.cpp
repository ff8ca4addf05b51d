// mcl.cpp -- the device driver of the homolog-group path (include/peprml.h "Homolog groups"): pml_mcl_cluster, pml_homolog_groups,
// pml_debug_mcl_steps, pml_mcl_stats.  The kernels are mcl.hip; the graph front end, the reading's union-find and ordering and
// the Java's filters mcl_host.cpp.  One CSR of the mirrored graph, the best rows and the masks are resident for the call; the
// components are sorted into their classes and worked through in sub-batches whose dense matrices fit the HBM budget, taken from
// the context's cached arena.  The host sees two ints per column, the masks, and for the HBM class one flag per component and
// iteration -- never a matrix.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <map>

#include "../../include/peprml.h"
#include "api_types.hpp"
#include "trim_dev.hpp"

using namespace pml;

namespace {

#define MCHK(expr)                                                                                                    \
    do { hipError_t e_ = (expr);                                                                                      \
         if (e_ != hipSuccess) return ctx->fail(PML_EDEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); } while (0)

struct DevBuf {
    char *d = nullptr;
    ~DevBuf() { if (d) hipFree(d); }
};

// the sub-batches' memory: the context's cached arena when it is large enough, else a new one that replaces it
struct Arena {
    Ctx *ctx; char *d = nullptr; size_t bytes = 0;
    explicit Arena(Ctx *c) : ctx(c) {}
    hipError_t take(size_t need) {
        if (ctx->arena_cache && ctx->arena_cache_bytes >= need) { d = ctx->arena_cache; bytes = ctx->arena_cache_bytes; ctx->arena_cache = nullptr; ctx->arena_cache_bytes = 0; return hipSuccess; }
        if (ctx->arena_cache) { hipFree(ctx->arena_cache); ctx->arena_cache = nullptr; ctx->arena_cache_bytes = 0; }
        bytes = std::max<size_t>(need, 256);
        return hipMalloc((void **)&d, bytes);
    }
    ~Arena() {
        if (!d) return;
        if (ctx->arena_cache_bytes < bytes) { if (ctx->arena_cache) hipFree(ctx->arena_cache); ctx->arena_cache = d; ctx->arena_cache_bytes = bytes; }
        else hipFree(d);
    }
};

int mcl_class_of(int n) { return n <= MCL_PACKED_MAX ? 0 : n <= MCL_LDS_MAX ? 1 : 2; }
int mcl_npad(int cls, int n) { return cls == 2 ? (n + MCL_TILE - 1) / MCL_TILE * MCL_TILE : n; }
size_t mcl_pool_doubles(int cls, int n) {
    const size_t np = (size_t)mcl_npad(cls, n);
    return align_up((cls == 2 ? 2 : 1) * np * np, 32);
}
constexpr size_t MCL_COMP_FIXED = sizeof(MclComp) + 32;          // its record, iteration count, chaos, flag and place in the active list
constexpr int MCL_SUB_MAX = 32768;                               // components of a sub-batch: a grid dimension

// the call's resident arrays
struct CallDev {
    DevBuf buf;
    long long *ptr = nullptr; int *row = nullptr; double *val = nullptr; int *best = nullptr; unsigned *mask = nullptr; double *chaos_col = nullptr;
};

struct Sub { int cls = 0; std::vector<MclComp> comps; std::vector<int> index; size_t pool = 0; int max_n = 0; };

size_t sub_bytes(size_t pool_doubles, size_t ncomps) { return pool_doubles * sizeof(double) + ncomps * MCL_COMP_FIXED + TRIM_BATCH_SLACK; }

// one sub-batch through its class.  dense_in (test door): the pool's content instead of k_mcl_fill's; write_back / pool_out: the
// final matrices
int run_sub(Ctx *ctx, Arena &ar, const Sub &sb, const MclRun &run, const CallDev &cd, const double *dense_in, std::vector<double> *pool_out, int *iters_out,
            double *chaos_out) {
    const size_t C = sb.comps.size();
    if (!C) return PML_OK;
    size_t off = 0;
    const size_t o_pool = off; off += align_up(sb.pool * sizeof(double), 256);
    const size_t o_comps = off; off += align_up(C * sizeof(MclComp), 256);
    const size_t o_iters = off; off += align_up(C * sizeof(int), 256);
    const size_t o_chaos = off; off += align_up(C * sizeof(double), 256);
    const size_t o_flag = off; off += align_up(C * sizeof(int), 256);
    const size_t o_active = off; off += align_up(C * sizeof(int), 256);
    if (off > ar.bytes) return ctx->fail(PML_EDEVICE, "internal: a sub-batch of " + std::to_string(off) + " bytes was planned into an arena of " + std::to_string(ar.bytes));
    char *d = ar.d;
    double *pool = (double *)(d + o_pool);
    const MclComp *comps = (const MclComp *)(d + o_comps);
    int *iters = (int *)(d + o_iters), *flag = (int *)(d + o_flag), *active = (int *)(d + o_active);
    double *chaos = (double *)(d + o_chaos);
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    if (ctx->profile) for (auto &e : ev) e = ctx->get_event();
    struct Back { Ctx *c; hipEvent_t *e; ~Back() { for (int i = 0; i < 3; ++i) if (e[i]) c->pool.push_back(e[i]); } } back{ctx, ev};
    if (ev[0]) hipEventRecord(ev[0], ctx->stream);
    MCHK(hipMemcpyAsync(d + o_comps, sb.comps.data(), C * sizeof(MclComp), hipMemcpyHostToDevice, ctx->stream));
    MCHK(hipMemsetAsync(d + o_iters, 0, o_active - o_iters, ctx->stream));
    if (dense_in) MCHK(hipMemcpyAsync(pool, dense_in, sb.pool * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    else {
        MCHK(hipMemsetAsync(pool, 0, sb.pool * sizeof(double), ctx->stream));
        launch_mcl_fill(comps, (int)C, sb.max_n, cd.ptr, cd.row, cd.val, pool, ctx->stream);
        ctx->mcl_launches[0]++;
    }
    if (ev[1]) hipEventRecord(ev[1], ctx->stream);
    ctx->mcl_launches[7]++;
    std::vector<int> h_iters(C, 0);
    if (sb.cls < 2) {
        MCHK(launch_mcl_lds(sb.cls == 0, comps, (int)C, pool, run, cd.best, cd.mask, iters, chaos, pool_out != nullptr, ctx->stream));
        ctx->mcl_launches[1 + sb.cls]++;
    } else {
        std::vector<int> act(C), h_flag(C);
        for (size_t i = 0; i < C; ++i) act[i] = (int)i;
        bool upload = true;
        for (int it = 0; it < run.max_iter && !act.empty(); ++it) {
            const int na = (int)act.size();
            int max_n = 0;
            for (int i : act) max_n = std::max(max_n, sb.comps[(size_t)i].n);
            if (upload) MCHK(hipMemcpyAsync(active, act.data(), (size_t)na * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
            launch_mcl_expand(comps, active, na, mcl_npad(2, max_n), pool, it & 1, ctx->stream);
            launch_mcl_inflate(comps, active, na, max_n, pool, it & 1, run, cd.chaos_col, ctx->stream);
            launch_mcl_flag(comps, active, na, cd.chaos_col, run, it + 1, iters, chaos, flag, ctx->stream);
            ctx->mcl_launches[3]++; ctx->mcl_launches[4]++; ctx->mcl_launches[5]++;
            MCHK(hipGetLastError());
            MCHK(hipMemcpyAsync(h_flag.data(), flag, (size_t)na * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
            if (ctx->sync(ctx->stream)) return PML_EDEVICE;
            size_t keep = 0;
            for (int i = 0; i < na; ++i) if (!h_flag[(size_t)i]) act[keep++] = act[(size_t)i];      // converged components drop out
            upload = keep != (size_t)na;
            act.resize(keep);
        }
        launch_mcl_read(comps, (int)C, sb.max_n, pool, iters, cd.best, cd.mask, ctx->stream);
        ctx->mcl_launches[6]++;
    }
    if (ev[2]) hipEventRecord(ev[2], ctx->stream);
    MCHK(hipGetLastError());
    MCHK(hipMemcpyAsync(h_iters.data(), iters, C * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    std::vector<double> h_chaos(C, 0.0);
    MCHK(hipMemcpyAsync(h_chaos.data(), chaos, C * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (pool_out) { pool_out->resize(sb.pool); MCHK(hipMemcpyAsync(pool_out->data(), pool, sb.pool * sizeof(double), hipMemcpyDeviceToHost, ctx->stream)); }
    if (ctx->sync(ctx->stream)) return PML_EDEVICE;
    if (ev[0]) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) ctx->mcl_ms[0] += ms;
        if (hipEventElapsedTime(&ms, ev[1], ev[2]) == hipSuccess) ctx->mcl_ms[1 + sb.cls] += ms;
    }
    for (size_t i = 0; i < C; ++i) {
        if (h_iters[i] < 0 || h_iters[i] > run.max_iter) return ctx->fail(PML_EDEVICE, "internal: a component reports " + std::to_string(h_iters[i]) + " iterations");
        if (iters_out) iters_out[i] = h_iters[i];
        if (chaos_out) chaos_out[i] = h_chaos[i];
    }
    return PML_OK;
}

MclRun run_of(const MclOpts &o) { MclRun r; r.inflation = o.inflation; r.prune_inverse = o.prune_inverse; r.chaos_eps = o.chaos_eps; r.max_iter = o.max_iter; r.pad = 0; return r; }

int check_opts(Ctx *ctx, const MclOpts &o) {
    if (!(o.inflation > 0) || !std::isfinite(o.inflation)) return ctx->fail(PML_EINVAL, "the inflation must be finite and > 0");
    if (!(o.prune_inverse > 0) || !std::isfinite(o.prune_inverse)) return ctx->fail(PML_EINVAL, "prune_inverse must be finite and > 0");
    if (o.max_iter < 1) return ctx->fail(PML_EINVAL, "max_iter must be at least 1");
    return PML_OK;
}

// every component of g through the kernels: best rows and masks as mcl_finish reads them
int cluster_graph(Ctx *ctx, const MclGraph &g, const MclOpts &o, std::vector<int> &best, std::vector<unsigned> &mask, int &iters) {
    const int N = g.n, NC = g.ncomp();
    iters = 0;
    best.assign((size_t)N, -1);
    std::vector<long long> mask_off((size_t)NC + 1, 0);
    for (int c = 0; c < NC; ++c) mask_off[(size_t)c + 1] = mask_off[(size_t)c] + (long long)g.size(c) * mcl_words(g.size(c));
    mask.assign((size_t)mask_off[(size_t)NC], 0u);
    if (!N) return PML_OK;
    MCHK(hipSetDevice(ctx->device));
    const size_t budget = trim_hbm_budget(ctx) + (std::getenv("PML_HBM_BUDGET_MB") ? 0 : ctx->arena_cache_bytes);     // the cached arena is reused or replaced
    const size_t nnz = g.row.size();
    CallDev cd;
    size_t off = 0;
    const size_t o_ptr = off; off += align_up(((size_t)N + 1) * sizeof(long long), 256);
    const size_t o_val = off; off += align_up(nnz * sizeof(double), 256);
    const size_t o_chaos = off; off += align_up((size_t)N * sizeof(double), 256);
    const size_t o_row = off; off += align_up(nnz * sizeof(int), 256);
    const size_t o_best = off; off += align_up((size_t)N * sizeof(int), 256);
    const size_t o_mask = off; off += align_up(mask.size() * sizeof(unsigned), 256);
    if (off > budget) return ctx->fail(PML_ENOMEM, "the graph's " + std::to_string(nnz) + " arcs and " + std::to_string(mask.size()) + " mask words need " +
                                                       std::to_string((off >> 20) + 1) + " MiB of HBM, the budget is " + std::to_string(budget >> 20) + " MiB");
    const size_t left = budget - off;
    // the sub-batches, class by class
    std::vector<Sub> subs;
    size_t arena_need = 0;
    for (int cls = 0; cls < 3; ++cls) {
        Sub cur; cur.cls = cls;
        auto flush = [&] { if (!cur.comps.empty()) { arena_need = std::max(arena_need, sub_bytes(cur.pool, cur.comps.size()) + 6 * 256); subs.push_back(std::move(cur)); } cur = Sub(); cur.cls = cls; };
        for (int c = 0; c < NC; ++c) {
            const int n = g.size(c);
            if (mcl_class_of(n) != cls) continue;
            const size_t pd = mcl_pool_doubles(cls, n);
            if (sub_bytes(pd, 1) + 6 * 256 > left)
                return ctx->fail(PML_ENOMEM, "a component of " + std::to_string(n) + " nodes needs " + std::to_string(((pd * sizeof(double)) >> 20) + 1) +
                                                 " MiB of HBM for its dense matrices, " + std::to_string(left >> 20) + " MiB of the budget of " + std::to_string(budget >> 20) +
                                                 " MiB are left; sparse expansion is not built");
            if (sub_bytes(cur.pool + pd, cur.comps.size() + 1) + 6 * 256 > left || (int)cur.comps.size() == MCL_SUB_MAX) flush();
            MclComp mc; mc.mat = (long long)cur.pool; mc.n = n; mc.npad = mcl_npad(cls, n); mc.col0 = g.comp_off[(size_t)c]; mc.pad = 0; mc.mask_off = mask_off[(size_t)c];
            cur.comps.push_back(mc); cur.index.push_back(c); cur.pool += pd; cur.max_n = std::max(cur.max_n, n);
        }
        flush();
    }
    MCHK(hipMalloc((void **)&cd.buf.d, std::max<size_t>(off, 256)));
    char *d = cd.buf.d;
    cd.ptr = (long long *)(d + o_ptr); cd.val = (double *)(d + o_val); cd.chaos_col = (double *)(d + o_chaos); cd.row = (int *)(d + o_row);
    cd.best = (int *)(d + o_best); cd.mask = (unsigned *)(d + o_mask);
    Arena ar(ctx);
    MCHK(ar.take(arena_need));
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (ctx->profile) { e0 = ctx->get_event(); e1 = ctx->get_event(); hipEventRecord(e0, ctx->stream); }
    MCHK(hipMemcpyAsync(cd.ptr, g.ptr.data(), ((size_t)N + 1) * sizeof(long long), hipMemcpyHostToDevice, ctx->stream));
    if (nnz) {
        MCHK(hipMemcpyAsync(cd.row, g.row.data(), nnz * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
        MCHK(hipMemcpyAsync(cd.val, g.val.data(), nnz * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    }
    MCHK(hipMemsetAsync(d + o_best, 0xFF, (o_mask - o_best) , ctx->stream));
    MCHK(hipMemsetAsync(d + o_mask, 0, std::max<size_t>(off - o_mask, 0), ctx->stream));
    if (e1) hipEventRecord(e1, ctx->stream);
    const MclRun run = run_of(o);
    int rc = PML_OK;
    std::vector<int> sub_iters;
    for (const Sub &sb : subs) {
        sub_iters.assign(sb.comps.size(), 0);
        if ((rc = run_sub(ctx, ar, sb, run, cd, nullptr, nullptr, sub_iters.data(), nullptr))) break;
        for (int it : sub_iters) iters = std::max(iters, it);
    }
    if (!rc) {
        hipError_t e = hipMemcpyAsync(best.data(), cd.best, (size_t)N * sizeof(int), hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess && !mask.empty()) e = hipMemcpyAsync(mask.data(), cd.mask, mask.size() * sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream);
        if (e != hipSuccess) rc = ctx->fail(PML_EDEVICE, std::string("reading the results: ") + hipGetErrorString(e));
        else if (ctx->sync(ctx->stream)) rc = PML_EDEVICE;
    }
    if (e0) {
        float ms = 0;
        if (!rc && hipEventElapsedTime(&ms, e0, e1) == hipSuccess) ctx->mcl_ms[0] += ms;
        ctx->pool.push_back(e0); ctx->pool.push_back(e1);
    }
    if (rc) return rc;
    for (int c = 0; c < NC; ++c)                                     // what came back is used as an index
        for (int j = 0; j < g.size(c); ++j) {
            const int b = best[(size_t)(g.comp_off[(size_t)c] + j)];
            if (b < -1 || b >= g.size(c)) return ctx->fail(PML_EDEVICE, "internal: a column's best row is " + std::to_string(b) + " in a component of " + std::to_string(g.size(c)));
        }
    return PML_OK;
}

template <class F> int guarded(pml_ctx *pctx, F f) {
    std::lock_guard<std::mutex> lk(pctx->c.mu);
    pml_fpguard fpg;
    pml_drop_worker_caches(pctx);
    try { return f(&pctx->c); }
    catch (const std::bad_alloc &) { return pctx->c.fail(PML_ENOMEM, "host allocation failed"); }
    catch (const std::exception &e) { return pctx->c.fail(PML_EINVAL, e.what()); }
}

int mcl_cluster(Ctx *ctx, int n, long long narcs, const int *a, const int *b, const double *w, const MclOpts &o, int *cluster_of, int *nclusters, int *iters, int *ncomp) {
    if (int rc = check_opts(ctx, o)) return rc;
    MclGraph g; std::string err;
    if (!mcl_build_graph(n, narcs, a, b, w, g, err)) return ctx->fail(PML_EINVAL, err);
    std::vector<int> best; std::vector<unsigned> mask; int it = 0;
    if (int rc = cluster_graph(ctx, g, o, best, mask, it)) return rc;
    mcl_finish(g, best.data(), mask.data(), cluster_of, nclusters);
    if (iters) *iters = it;
    if (ncomp) *ncomp = g.ncomp();
    return PML_OK;
}

char *dup_string(const std::string &s) { char *p = (char *)std::malloc(s.size() + 1); if (p) std::memcpy(p, s.c_str(), s.size() + 1); return p; }

int homolog_groups(Ctx *ctx, const pml_homolog_groups_opts &o, pml_homolog_groups_result *res) {
    if (o.score_field != 2 && o.score_field != 11) return ctx->fail(PML_EINVAL, "score_field is 2 or 11");
    if (o.score_field == 2 && o.bidirectional) return ctx->fail(PML_EINVAL, "the bidirectional filter reads field 11: score_field must be 11");
    if (o.table_bytes < 0 || (o.table_bytes > 0 && !o.table)) return ctx->fail(PML_EINVAL, "the hit table is missing");
    if (o.ntaxon_labels < 0 || (o.ntaxon_labels > 0 && (!o.taxon_labels || !o.taxon_of))) return ctx->fail(PML_EINVAL, "the taxon list is malformed");
    std::string filtered, err;
    const char *abc = o.table; size_t abc_n = (size_t)o.table_bytes;
    if (o.score_field == 11) {
        if (o.bidirectional) hits_bidirectional(o.table, (size_t)o.table_bytes, 11, filtered);
        else if (!hits_filter(o.table, (size_t)o.table_bytes, filtered, err)) return ctx->fail(PML_EINVAL, err);
        abc = filtered.data(); abc_n = filtered.size();
    }
    std::vector<std::string> labels; std::vector<int> a, b; std::vector<double> w;
    if (!abc_parse(abc, abc_n, labels, a, b, w, err)) return ctx->fail(PML_EINVAL, err);
    const int n = (int)labels.size();
    std::vector<int> cluster_of((size_t)n, 0);
    int ncl = 0, iters = 0, ncomp = 0;
    if (int rc = mcl_cluster(ctx, n, (long long)a.size(), a.data(), b.data(), w.data(), mcl_resolve(&o.mcl), cluster_of.data(), &ncl, &iters, &ncomp)) return rc;
    std::vector<long long> offs((size_t)ncl + 1, 0);
    for (int i = 0; i < n; ++i) offs[(size_t)cluster_of[(size_t)i] + 1]++;
    for (int k = 0; k < ncl; ++k) offs[(size_t)k + 1] += offs[(size_t)k];
    std::vector<int> members((size_t)n), at(offs.begin(), offs.end() - 1);
    for (int i = 0; i < n; ++i) members[(size_t)at[(size_t)cluster_of[(size_t)i]]++] = i;          // ascending inside a cluster
    std::string text;
    for (int k = 0; k < ncl; ++k)
        for (long long i = offs[(size_t)k]; i < offs[(size_t)k + 1]; ++i) { text += labels[(size_t)members[(size_t)i]]; text += i + 1 < offs[(size_t)k + 1] ? '\t' : '\n'; }
    std::vector<int> kept;
    if (o.ntaxon_labels > 0) {
        std::map<std::string, int> taxon;
        for (int i = 0; i < o.ntaxon_labels; ++i) { if (!o.taxon_labels[i]) return ctx->fail(PML_EINVAL, "a null taxon label"); taxon[o.taxon_labels[i]] = o.taxon_of[i]; }
        std::vector<int> taxon_of_node((size_t)n);
        for (int i = 0; i < n; ++i) {
            auto it = taxon.find(labels[(size_t)i]);
            if (it == taxon.end()) return ctx->fail(PML_EINVAL, "the label '" + labels[(size_t)i] + "' of the hit table has no taxon");
            taxon_of_node[(size_t)i] = it->second;
        }
        homolog_select(ncl, offs.data(), members.data(), taxon_of_node.data(), o.min_taxa, o.max_taxa, o.rep_only != 0, o.target_ntax, o.target_min_gene, kept);
    } else for (int k = 0; k < ncl; ++k) kept.push_back(k);
    res->nlabels = n; res->nclusters = ncl; res->nkept = (int)kept.size(); res->ncomponents = ncomp; res->iterations = iters;
    res->labels = (char **)std::calloc((size_t)std::max(n, 1), sizeof(char *));
    res->cluster_off = (long long *)std::malloc(sizeof(long long) * ((size_t)ncl + 1));
    res->members = (int *)std::malloc(sizeof(int) * (size_t)std::max(n, 1));
    res->kept = (int *)std::malloc(sizeof(int) * std::max<size_t>(kept.size(), 1));
    res->mcl_text = dup_string(text);
    if (o.score_field == 11) res->filtered_text = dup_string(filtered);
    if (!res->labels || !res->cluster_off || !res->members || !res->kept || !res->mcl_text || (o.score_field == 11 && !res->filtered_text)) return ctx->fail(PML_ENOMEM, "host allocation failed");
    for (int i = 0; i < n; ++i) if (!(res->labels[i] = dup_string(labels[(size_t)i]))) return ctx->fail(PML_ENOMEM, "host allocation failed");
    std::copy(offs.begin(), offs.end(), res->cluster_off);
    std::copy(members.begin(), members.end(), res->members);
    std::copy(kept.begin(), kept.end(), res->kept);
    return PML_OK;
}

}  // namespace

extern "C" int pml_mcl_cluster(pml_ctx *pctx, int n, long long narcs, const int *a, const int *b, const double *w, const pml_mcl_opts *opts, int *cluster_of_out,
                               int *nclusters_out, int *iters_out) {
    if (!pctx || n < 0 || narcs < 0 || (narcs > 0 && (!a || !b || !w)) || (n > 0 && !cluster_of_out) || !nclusters_out) return PML_EINVAL;
    return guarded(pctx, [&](Ctx *ctx) -> int { return mcl_cluster(ctx, n, narcs, a, b, w, mcl_resolve(opts), cluster_of_out, nclusters_out, iters_out, nullptr); });
}

extern "C" void pml_homolog_groups_result_free(pml_homolog_groups_result *r) {
    if (!r) return;
    if (r->labels) for (int i = 0; i < r->nlabels; ++i) std::free(r->labels[i]);
    std::free(r->labels); std::free(r->cluster_off); std::free(r->members); std::free(r->mcl_text); std::free(r->kept); std::free(r->filtered_text);
    std::memset(r, 0, sizeof *r);
}

extern "C" int pml_homolog_groups(pml_ctx *pctx, const pml_homolog_groups_opts *opts, pml_homolog_groups_result *result) {
    if (result) std::memset(result, 0, sizeof *result);
    if (!pctx || !opts || !result) return PML_EINVAL;
    const int rc = guarded(pctx, [&](Ctx *ctx) -> int { return homolog_groups(ctx, *opts, result); });
    if (rc) pml_homolog_groups_result_free(result);
    return rc;
}

extern "C" int pml_debug_mcl_steps(pml_ctx *pctx, int n, const double *matrix_in, const pml_mcl_opts *opts, int nsteps, int force_class, double *matrix_out,
                                   double *chaos_out) {
    if (!pctx || n < 1 || !matrix_in || nsteps < 1 || force_class < 0 || force_class > 2 || !matrix_out) return PML_EINVAL;
    return guarded(pctx, [&](Ctx *ctx) -> int {
        MclOpts o = mcl_resolve(opts);
        if (int rc = check_opts(ctx, o)) return rc;
        if ((force_class == 0 && n > MCL_PACKED_MAX) || (force_class == 1 && n > MCL_LDS_MAX))
            return ctx->fail(PML_EINVAL, "a component of " + std::to_string(n) + " nodes does not fit class " + std::to_string(force_class));
        o.max_iter = nsteps; o.chaos_eps = -1.0;                     // chaos is never below it: no convergence test
        MCHK(hipSetDevice(ctx->device));
        Sub sb; sb.cls = force_class; sb.max_n = n; sb.pool = mcl_pool_doubles(force_class, n);
        MclComp mc; mc.mat = 0; mc.n = n; mc.npad = mcl_npad(force_class, n); mc.col0 = 0; mc.pad = 0; mc.mask_off = 0;
        sb.comps.push_back(mc); sb.index.push_back(0);
        const size_t need = sub_bytes(sb.pool, 1) + 6 * 256, W = (size_t)mcl_words(n);
        if (need + (size_t)n * (12 + 4 * W) + 1024 > trim_hbm_budget(ctx) + (std::getenv("PML_HBM_BUDGET_MB") ? 0 : ctx->arena_cache_bytes)) return ctx->fail(PML_ENOMEM, "the component does not fit the HBM budget");
        CallDev cd;
        size_t off = 0;
        const size_t o_chaos = off; off += align_up((size_t)n * sizeof(double), 256);
        const size_t o_best = off; off += align_up((size_t)n * sizeof(int), 256);
        const size_t o_mask = off; off += align_up((size_t)n * W * sizeof(unsigned), 256);
        MCHK(hipMalloc((void **)&cd.buf.d, off));
        cd.chaos_col = (double *)(cd.buf.d + o_chaos); cd.best = (int *)(cd.buf.d + o_best); cd.mask = (unsigned *)(cd.buf.d + o_mask);
        Arena ar(ctx);
        MCHK(ar.take(need));
        const size_t ld = (size_t)mc.npad;
        std::vector<double> in(sb.pool, 0.0), out;
        for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) in[(size_t)j * ld + i] = matrix_in[(size_t)i * n + j];
        int iters = 0; double chaos = 0;
        if (int rc = run_sub(ctx, ar, sb, run_of(o), cd, in.data(), &out, &iters, &chaos)) return rc;
        const size_t base = force_class == 2 && (iters & 1) ? ld * ld : 0;
        for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) matrix_out[(size_t)i * n + j] = out[base + (size_t)j * ld + i];
        if (chaos_out) *chaos_out = chaos;
        return PML_OK;
    });
}

extern "C" int pml_mcl_stats(pml_ctx *ctx, long long *launches, double *total_ms) {
    if (!ctx) return PML_EINVAL;
    std::lock_guard<std::mutex> lk(ctx->c.mu);
    if (launches) for (int i = 0; i < 8; ++i) launches[i] = ctx->c.mcl_launches[i];
    if (total_ms) for (int i = 0; i < 4; ++i) total_ms[i] = ctx->c.mcl_ms[i];
    return PML_OK;
}
