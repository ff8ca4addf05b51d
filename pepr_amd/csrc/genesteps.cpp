// genesteps.cpp -- the device-driving half of the gene homoplasy test (include/peprml.h): pml_gene_steps, pml_step_thresholds,
// pml_debug_step_replicates, pml_gene_steps_stats.  The kernels are genesteps.hip; the option checks, domains, draws, totals and
// the order statistic are genesteps_host.cpp.
// A sub-batch of genes is resident as a GeneStore (the encoded patterns k_fitch_tips reads) and ONE further allocation: the
// genes' raw bytes in the CgGene layout and their site2pat maps, the Fitch pool of the replicate of all genes of the sub-batch
// (tips and one vector per inner node), the pattern counts and the two per-column outputs.
#include <algorithm>
#include <climits>
#include <cstdlib>
#include <cstring>

#include "../../include/peprml.h"
#include "api_types.hpp"
#include "fitch_dev.hpp"
#include "genesteps.hpp"

using namespace pml;

namespace {
#define GSCHK(expr)                                                                                                   \
    do { hipError_t e_ = (expr);                                                                                      \
         if (e_ != hipSuccess) return ctx->fail(PML_EDEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); } while (0)

size_t hbm_budget(Ctx *ctx) {
    hipSetDevice(ctx->device);
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = (size_t)1 << 40;
    size_t budget = (size_t)(0.85 * (double)free_b);
    if (const char *e = std::getenv("PML_HBM_BUDGET_MB")) budget = (size_t)std::atoll(e) << 20;
    return budget;
}

// what one gene adds to a sub-batch at most (its patterns are not known before it is encoded: npat <= ncols): the store's codes
// and weights, raw bytes, site2pat, steps, min_steps, pattern counts and weights, its share of the pool, tiles and descriptors
size_t gene_cost(int ntax, int ncols, int n_union) {
    const size_t ld = align_up((size_t)ncols, 16), mp = (size_t)ncols + 32;
    size_t b = align_up((size_t)ntax * mp, 256) + align_up(mp * 8, 256);
    b += align_up((size_t)ntax * ld, 256) + align_up((size_t)ncols * sizeof(int), 256) + 4 * sizeof(int) * (size_t)ncols;
    b += (size_t)(2 * n_union - 2) * sizeof(unsigned) * (size_t)ncols;
    b += sizeof(int) * (size_t)((ncols + GS_COLS - 1) / GS_COLS) + sizeof(GsGene) + sizeof(FTipSeg) + 2 * sizeof(int) + sizeof(int) * (size_t)n_union;
    return b;
}
// the shared arrays' own alignment, the operation list, and the pool's padding to 32 patterns
size_t batch_fixed(int n_union) { return 16 * 256 + sizeof(GsOp) * (size_t)n_union + (size_t)(2 * n_union - 2) * sizeof(unsigned) * 64 + 64 * 2 * sizeof(int); }

struct Events {
    Ctx *c; hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
    explicit Events(Ctx *ctx) : c(ctx) { if (c->profile) for (auto &x : e) x = c->get_event(); }
    ~Events() { for (auto &x : e) if (x) c->pool.push_back(x); }
    void mark(int k) { if (e[k]) hipEventRecord(e[k], c->stream); }
    void add(int k0, int k1, double &ms) { float t = 0; if (e[k0] && hipEventElapsedTime(&t, e[k0], e[k1]) == hipSuccess) ms += t; }
};

// genes [first, first + ng) of the call: steps and min_steps of their columns into res (at col_start[first])
int run_batch(Ctx *ctx, const pml_alignment *genes, int first, int ng, const std::vector<std::string> &names, const std::vector<GsOp> &ops, pml_gene_steps_result *res) {
    const int n = (int)names.size();
    GeneStore store;
    struct Drop { GeneStore &s; ~Drop() { s.destroy(); } } drop{store};
    static_assert(sizeof(pml_alignment) == sizeof(pml_alignment_view), "alignment view layout");
    if (int rc = store.create(ctx, ng, reinterpret_cast<const pml_alignment_view *>(genes + first))) return rc;
    long long P = 0, C = 0, tiles = 0; int max_npat = 0;
    std::vector<size_t> ld((size_t)ng), o_bytes((size_t)ng), o_s2p((size_t)ng);
    std::vector<int> pat_off((size_t)ng);
    for (int i = 0; i < ng; ++i) {
        const EncodedAlignment &A = store.items[(size_t)i].aln;
        pat_off[(size_t)i] = (int)P; P += A.npat; C += A.nsites; tiles += (A.nsites + GS_COLS - 1) / GS_COLS;
        max_npat = std::max(max_npat, A.npat); ld[(size_t)i] = align_up((size_t)A.nsites, 16);
    }
    if (P > INT_MAX - 64 || tiles > INT_MAX) return ctx->fail(PML_EINVAL, "too many columns for one sub-batch");
    const int mpad = std::max(32, (int)((P + 31) / 32 * 32)), ntiles = (int)tiles;
    size_t off = align_up((size_t)ng * sizeof(GsGene), 256);
    const size_t o_tiles = off; off += align_up((size_t)ntiles * sizeof(int), 256);
    const size_t o_first = off; off += align_up((size_t)ng * sizeof(int), 256);
    const size_t o_ops = off; off += align_up(ops.size() * sizeof(GsOp), 256);
    const size_t o_segs = off; off += align_up((size_t)ng * sizeof(FTipSeg), 256);
    const size_t o_maps = off; off += align_up((size_t)ng * n * sizeof(int), 256);
    for (int i = 0; i < ng; ++i) {
        o_s2p[(size_t)i] = off; off += align_up((size_t)genes[first + i].nsites * sizeof(int), 256);
        o_bytes[(size_t)i] = off; off += align_up((size_t)genes[first + i].ntax * ld[(size_t)i], 256);
    }
    const size_t in_bytes = off;
    const size_t o_w = off; off += align_up((size_t)mpad * sizeof(int), 256);
    const size_t o_pat = off; off += align_up((size_t)mpad * sizeof(int), 256);
    const size_t o_steps = off; off += align_up((size_t)C * sizeof(int), 256);
    const size_t o_mins = off; off += align_up((size_t)C * sizeof(int), 256);
    const size_t o_pool = off; off += (size_t)(2 * n - 2) * mpad * sizeof(unsigned);
    char *d = nullptr;
    GSCHK(hipMalloc((void **)&d, off));
    struct Free { char *p; ~Free() { hipFree(p); } } freer{d};
    std::vector<char> host(in_bytes, 0);
    int *tile_gene = (int *)(host.data() + o_tiles), *tile_first = (int *)(host.data() + o_first), *maps = (int *)(host.data() + o_maps);
    std::memcpy(host.data() + o_ops, ops.data(), ops.size() * sizeof(GsOp));
    std::fill(maps, maps + (size_t)ng * n, -1);
    long long col_base = 0; int t = 0;
    for (int i = 0; i < ng; ++i) {
        const pml_alignment &A = genes[first + i];
        const GeneStore::Item &it = store.items[(size_t)i];
        for (int r = 0; r < A.ntax; ++r) {
            std::memcpy(host.data() + o_bytes[(size_t)i] + (size_t)r * ld[(size_t)i], A.rows[r], (size_t)A.nsites);      // the store has checked the rows' lengths
            maps[(size_t)i * n + (size_t)(std::lower_bound(names.begin(), names.end(), it.aln.names[(size_t)r]) - names.begin())] = r;
        }
        if (A.nsites) std::memcpy(host.data() + o_s2p[(size_t)i], it.aln.site2pat.data(), (size_t)A.nsites * sizeof(int));
        ((GsGene *)host.data())[i] = GsGene{(const uint8_t *)(d + o_bytes[(size_t)i]), (const int *)(d + o_s2p[(size_t)i]), A.ntax, A.nsites, (int)ld[(size_t)i], pat_off[(size_t)i], col_base};
        ((FTipSeg *)(host.data() + o_segs))[i] = FTipSeg{it.d_codes, it.d_w, (const int *)(d + o_maps) + (size_t)i * n, (unsigned *)(d + o_pool), (int *)(d + o_w),
                                                          it.aln.mpad, it.aln.npat, mpad, pat_off[(size_t)i], n, 0};
        tile_first[i] = t;
        for (int k = 0; k < (A.nsites + GS_COLS - 1) / GS_COLS; ++k) tile_gene[t++] = i;
        col_base += A.nsites;
    }
    Events ev(ctx);
    GSCHK(hipMemcpyAsync(d, host.data(), in_bytes, hipMemcpyHostToDevice, ctx->stream));
    launch_fitch_tips((const FTipSeg *)(d + o_segs), ng, max_npat, ctx->stream);
    if (max_npat > 0) ctx->fitch_tips_launches++;
    ev.mark(0);
    launch_fitch_sitesteps((const GsOp *)(d + o_ops), (int)ops.size(), (unsigned *)(d + o_pool), mpad, (int)P, (int *)(d + o_pat), ctx->stream);
    ev.mark(1);
    launch_steps_expand((const GsGene *)d, (const int *)(d + o_tiles), (const int *)(d + o_first), ntiles, (const int *)(d + o_pat), (int *)(d + o_steps), ctx->stream);
    ev.mark(2);
    launch_colminsteps((const GsGene *)d, (const int *)(d + o_tiles), (const int *)(d + o_first), ntiles, n, (int *)(d + o_mins), ctx->stream);
    ev.mark(3);
    GSCHK(hipGetLastError());
    if (P > 0) ctx->gs_launches[0]++;
    if (ntiles > 0) { ctx->gs_launches[1]++; ctx->gs_launches[2]++; }
    const long long c0 = res->col_start[first];
    if (C) {
        GSCHK(hipMemcpyAsync(res->steps + c0, d + o_steps, (size_t)C * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        GSCHK(hipMemcpyAsync(res->min_steps + c0, d + o_mins, (size_t)C * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    }
    if (ctx->sync(ctx->stream)) return PML_EDEVICE;
    for (int k = 0; k < 3; ++k) ev.add(k, k + 1, ctx->gs_ms[k]);
    for (int i = 0; i < ng; ++i)
        for (long long c = res->col_start[first + i]; c < res->col_start[first + i + 1]; ++c)
            if (res->min_steps[c] < 0)
                return ctx->fail(PML_EPARSE, "gene " + std::to_string(first + i) + ", column " + std::to_string(c - res->col_start[first + i]) +
                                                 " holds nothing but '-' and '?' (the reference's getMinimumStepsPerSite dereferences null there)");
    return PML_OK;
}

int gene_steps_locked(pml_ctx *pctx, int ngenes, const pml_alignment *genes, const char *newick, pml_gene_steps_result *res) {
    Ctx *ctx = &pctx->c;
    std::vector<std::string> names;
    long long ncols = 0;
    for (int g = 0; g < ngenes; ++g) {
        const pml_alignment &A = genes[g];
        if (!A.names || !A.rows || A.ntax <= 0 || A.nsites < 0) return ctx->fail(PML_EINVAL, "bad alignment (gene " + std::to_string(g) + ")");
        std::vector<std::string> own;
        for (int i = 0; i < A.ntax; ++i) {
            if (!A.names[i] || !A.rows[i]) return ctx->fail(PML_EINVAL, "bad alignment (gene " + std::to_string(g) + ")");
            own.emplace_back(A.names[i]);
        }
        std::sort(own.begin(), own.end());
        if (std::adjacent_find(own.begin(), own.end()) != own.end()) return ctx->fail(PML_EINVAL, "gene " + std::to_string(g) + " names a taxon twice");
        names.insert(names.end(), own.begin(), own.end());
        ncols += A.nsites;
    }
    std::sort(names.begin(), names.end()); names.erase(std::unique(names.begin(), names.end()), names.end());
    const int n = (int)names.size();
    // the tree: exactly the union's taxa, binary but for a trifurcation (or a rooted bifurcation) at the top
    std::string err;
    std::vector<RawNode> raw;
    if (!parse_newick_raw(newick, raw, err)) return ctx->fail(PML_EPARSE, err);
    for (size_t v = 0; v < raw.size(); ++v) {
        const size_t k = raw[v].kids.size();
        if (k > 3 || (k == 3 && v != 0)) return ctx->fail(PML_EPARSE, "the tree has a polytomy other than the trifurcation at its top");
        if (k == 1) return ctx->fail(PML_EPARSE, "the tree has a node with a single child");
    }
    Tree tree;
    if (!Tree::parse(newick, names, tree, err)) return ctx->fail(PML_EPARSE, err);
    // post-order from tip 0: the reverse of a pre-order visits children before parents.  Vector ids: tip i = i, inner node v = v
    std::vector<GsOp> ops;
    {
        std::vector<std::pair<int, int>> stack{{tree.nbr[0][0], 0}};
        while (!stack.empty()) {
            const auto [v, from] = stack.back(); stack.pop_back();
            if (v < n) continue;
            const int k = tree.slot(v, from), x = tree.nbr[v][(k + 1) % 3], y = tree.nbr[v][(k + 2) % 3];
            ops.push_back(GsOp{v, x, y, 0});
            stack.push_back({x, v}); stack.push_back({y, v});
        }
        std::reverse(ops.begin(), ops.end());
        ops.push_back(GsOp{-1, tree.nbr[0][0], 0, 0});           // the edge to tip 0
    }
    std::memset(res, 0, sizeof *res);
    res->ngenes = ngenes; res->ntax = n; res->ncols = ncols;
    res->names = (char **)std::calloc((size_t)n, sizeof(char *));
    res->col_start = (long long *)std::calloc((size_t)ngenes + 1, sizeof(long long));
    res->steps = (int *)std::calloc((size_t)std::max<long long>(ncols, 1), sizeof(int));
    res->min_steps = (int *)std::calloc((size_t)std::max<long long>(ncols, 1), sizeof(int));
    res->gene_steps = (long long *)std::calloc((size_t)ngenes, sizeof(long long));
    res->gene_beyond = (long long *)std::calloc((size_t)ngenes, sizeof(long long));
    res->gene_ratio = (float *)std::calloc((size_t)ngenes, sizeof(float));
    if (!res->names || !res->col_start || !res->steps || !res->min_steps || !res->gene_steps || !res->gene_beyond || !res->gene_ratio)
        return ctx->fail(PML_ENOMEM, "host allocation failed");
    for (int i = 0; i < n; ++i) {
        if (!(res->names[i] = (char *)std::malloc(names[(size_t)i].size() + 1))) return ctx->fail(PML_ENOMEM, "host allocation failed");
        std::memcpy(res->names[i], names[(size_t)i].c_str(), names[(size_t)i].size() + 1);
    }
    for (int g = 0; g < ngenes; ++g) res->col_start[g + 1] = res->col_start[g] + genes[g].nsites;
    const size_t budget = hbm_budget(ctx);
    for (int g0 = 0; g0 < ngenes;) {
        size_t need = batch_fixed(n); int g1 = g0;
        while (g1 < ngenes) {
            const size_t c = gene_cost(genes[g1].ntax, genes[g1].nsites, n);
            if (need + c > budget) break;
            need += c; ++g1;
        }
        if (g1 == g0) {
            const size_t c = batch_fixed(n) + gene_cost(genes[g0].ntax, genes[g0].nsites, n);
            return ctx->fail(PML_ENOMEM, "gene " + std::to_string(g0) + " (" + std::to_string(genes[g0].ntax) + " rows, " + std::to_string(genes[g0].nsites) +
                                             " columns, " + std::to_string(n) + " taxa in the tree) needs " + std::to_string((c + ((size_t)1 << 20) - 1) >> 20) +
                                             " MiB of HBM for its bytes, patterns and Fitch vectors, the budget is " + std::to_string(budget >> 20) + " MiB");
        }
        if (int rc = run_batch(ctx, genes, g0, g1 - g0, names, ops, res)) return rc;
        g0 = g1;
    }
    gs_totals(ngenes, res->col_start, res->steps, res->min_steps, res->gene_steps, res->gene_beyond, res->gene_ratio);
    return PML_OK;
}

// the replicate sums of every gene (only < 0) or of one gene alone in its launch; thresholds and n_ge, or the unsorted sums
int thresholds_locked(Ctx *ctx, const pml_gene_steps_result *res, const pml_step_threshold_opts *opts, int only, double *threshold, long long *n_ge, double *sums_out) {
    if (res->ngenes < 1 || !res->col_start || !res->steps || !res->min_steps || !res->gene_steps || !res->gene_beyond || !res->gene_ratio)
        return ctx->fail(PML_EINVAL, "not a result of pml_gene_steps");
    const int G = res->ngenes;
    const GsOpts o{opts->statistic, opts->replace, opts->multiple, opts->reps, opts->alpha, opts->seed, opts->mask};
    GsPlan plan; std::string err;
    if (only >= G) return ctx->fail(PML_EINVAL, "gene index out of range");
    if (int rc = gs_plan(o, G, res->col_start, only, plan, err)) return ctx->fail(rc, err);
    if (only >= 0 && !plan.run[(size_t)only]) return ctx->fail(PML_EINVAL, "gene " + std::to_string(only) + " has too few columns to draw from: its threshold is -1, it has no replicates");
    const int reps = o.reps;
    const bool as_float = o.statistic == PML_STEPS_MIN_RATIO;
    std::vector<GsEntry> entries;
    for (int g = 0; g < G; ++g) {
        if (only >= 0 ? g != only : !plan.run[(size_t)g]) continue;
        entries.push_back(GsEntry{g, plan.len[(size_t)g], plan.U[(size_t)g], plan.split[(size_t)g]});
    }
    const size_t nT = plan.table_cols.size();
    std::vector<int> hs(2 * std::max<size_t>(nT, 1));
    for (size_t i = 0; i < nT; ++i) { hs[i] = res->steps[plan.table_cols[i]]; hs[nT + i] = res->min_steps[plan.table_cols[i]]; }
    const size_t chunk = std::max<size_t>(1, std::min<size_t>(std::max<size_t>(entries.size(), 1), ((size_t)1 << 26) / (size_t)reps));      // genes per launch: at most 2^26 sums
    const size_t o_tab = align_up(2 * nT * sizeof(int), 256), o_ent = o_tab + align_up(std::max<size_t>(nT, 1) * 4, 256),
                 o_sums = o_ent + align_up(chunk * sizeof(GsEntry), 256), bytes = o_sums + chunk * (size_t)reps * 4;
    GSCHK(hipSetDevice(ctx->device));
    char *d = nullptr;
    GSCHK(hipMalloc((void **)&d, bytes));
    struct Free { char *p; ~Free() { hipFree(p); } } freer{d};
    Events ev(ctx);
    if (nT) {
        GSCHK(hipMemcpyAsync(d, hs.data(), 2 * nT * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
        ev.mark(0);
        launch_steps_table((const int *)d, (const int *)d + nT, (long long)nT, o.statistic, d + o_tab, ctx->stream);
        ev.mark(1);
        ctx->gs_launches[4]++;
        GSCHK(hipGetLastError());
    }
    std::vector<int> raw(chunk * (size_t)reps);
    std::vector<double> sums((size_t)reps);
    for (int g = 0; only < 0 && g < G; ++g) if (!plan.run[(size_t)g]) { threshold[g] = -1; if (n_ge) n_ge[g] = -1; }
    for (size_t e0 = 0; e0 < entries.size(); e0 += chunk) {
        const size_t ne = std::min(chunk, entries.size() - e0);
        GSCHK(hipMemcpyAsync(d + o_ent, entries.data() + e0, ne * sizeof(GsEntry), hipMemcpyHostToDevice, ctx->stream));
        ev.mark(2);
        launch_steps_resample((const GsEntry *)(d + o_ent), (int)ne, d + o_tab, d + o_sums, reps, gs_base(o.seed), as_float, o.replace != 0, ctx->stream);
        ev.mark(3);
        ctx->gs_launches[3]++;
        GSCHK(hipGetLastError());
        GSCHK(hipMemcpyAsync(raw.data(), d + o_sums, ne * (size_t)reps * 4, hipMemcpyDeviceToHost, ctx->stream));
        if (ctx->sync(ctx->stream)) return PML_EDEVICE;
        ev.add(2, 3, ctx->gs_ms[3]);
        if (e0 == 0 && nT) ev.add(0, 1, ctx->gs_ms[4]);
        for (size_t i = 0; i < ne; ++i) {
            const int g = entries[e0 + i].gene;
            for (int b = 0; b < reps; ++b)
                sums[(size_t)b] = as_float ? (double)((const float *)raw.data())[i * (size_t)reps + (size_t)b] : (double)raw[i * (size_t)reps + (size_t)b];
            if (sums_out) { std::copy(sums.begin(), sums.end(), sums_out); continue; }
            const double observed = o.statistic == PML_STEPS_RAW ? (double)res->gene_steps[g] : o.statistic == PML_STEPS_BEYOND_MIN ? (double)res->gene_beyond[g] : (double)res->gene_ratio[g];
            threshold[g] = gs_order_statistic(sums.data(), reps, plan.k, observed, n_ge ? &n_ge[g] : nullptr);
        }
    }
    return PML_OK;
}
}  // namespace

extern "C" void pml_gene_steps_result_free(pml_gene_steps_result *r) {
    if (!r) return;
    if (r->names) for (int i = 0; i < r->ntax; ++i) std::free(r->names[i]);
    std::free(r->names); std::free(r->col_start); std::free(r->steps); std::free(r->min_steps);
    std::free(r->gene_steps); std::free(r->gene_beyond); std::free(r->gene_ratio);
    std::memset(r, 0, sizeof *r);
}

extern "C" int pml_gene_steps(pml_ctx *ctx, int ngenes, const pml_alignment *genes, const char *newick, pml_gene_steps_result *out) {
    if (out) std::memset(out, 0, sizeof *out);
    if (!ctx || !genes || ngenes < 1 || !newick || !out) return PML_EINVAL;
    std::lock_guard<std::mutex> lk(ctx->c.mu);
    pml_fpguard fpg;
    pml_drop_worker_caches(ctx);
    int rc;
    try { rc = gene_steps_locked(ctx, ngenes, genes, newick, out); }
    catch (const std::bad_alloc &) { rc = ctx->c.fail(PML_ENOMEM, "host allocation failed"); }
    catch (const std::exception &e) { rc = ctx->c.fail(PML_EINVAL, e.what()); }
    if (rc) pml_gene_steps_result_free(out);
    return rc;
}

extern "C" int pml_step_thresholds(pml_ctx *ctx, const pml_gene_steps_result *result, const pml_step_threshold_opts *opts, double *threshold, long long *n_ge) {
    if (!ctx || !result || !opts || !threshold) return PML_EINVAL;
    std::lock_guard<std::mutex> lk(ctx->c.mu);
    pml_fpguard fpg;
    pml_drop_worker_caches(ctx);
    try { return thresholds_locked(&ctx->c, result, opts, -1, threshold, n_ge, nullptr); }
    catch (const std::bad_alloc &) { return ctx->c.fail(PML_ENOMEM, "host allocation failed"); }
    catch (const std::exception &e) { return ctx->c.fail(PML_EINVAL, e.what()); }
}

extern "C" int pml_debug_step_replicates(pml_ctx *ctx, const pml_gene_steps_result *result, const pml_step_threshold_opts *opts, int gene, double *sums) {
    if (!ctx || !result || !opts || !sums || gene < 0) return PML_EINVAL;
    std::lock_guard<std::mutex> lk(ctx->c.mu);
    pml_fpguard fpg;
    pml_drop_worker_caches(ctx);
    try { return thresholds_locked(&ctx->c, result, opts, gene, nullptr, nullptr, sums); }
    catch (const std::bad_alloc &) { return ctx->c.fail(PML_ENOMEM, "host allocation failed"); }
    catch (const std::exception &e) { return ctx->c.fail(PML_EINVAL, e.what()); }
}

extern "C" int pml_gene_steps_stats(pml_ctx *ctx, long long *launches, double *total_ms) {
    if (!ctx) return PML_EINVAL;
    std::lock_guard<std::mutex> lk(ctx->c.mu);
    for (int k = 0; k < 5; ++k) { if (launches) launches[k] = ctx->c.gs_launches[k]; if (total_ms) total_ms[k] = ctx->c.gs_ms[k]; }
    return PML_OK;
}
