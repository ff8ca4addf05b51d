// treecmpapi.cpp -- the C ABI of the tree-set comparison (include/peprml.h): pml_tree_compare, pml_tree_compare_one and the two
// test doors.  The records come from treecmp.cpp (host), the kernels are treecmp.hip.  The records of all trees stay in HBM for
// the call; the pair outputs (32 bytes per pair) are produced in blocks of rows that fit the budget and finished on the host:
// the RF values from the integer counts, the two distances from the six sums with the host's sqrt and division.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>

#include "../../include/peprml.h"
#include "api_types.hpp"
#include "treecmp.hpp"

using namespace pml;

namespace {
#define TCCHK(expr)                                                                                                   \
    do { hipError_t e_ = (expr);                                                                                      \
         if (e_ != hipSuccess) return ctx->fail(PML_EDEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); } while (0)

unsigned long long pow2_at_least(unsigned long long x) { unsigned long long c = 64; while (c < x) c <<= 1; return c; }
constexpr int TC_MAX_ROWS = 32768;             // rows of one k_tree_pairs launch (grid.y)
constexpr size_t TC_MAX_BLOCK_BYTES = (size_t)1 << 30;      // pair outputs of one block of rows, whatever the budget allows

struct TreeCmp {
    Ctx *ctx = nullptr;
    TcSet S;
    int T = 0, maxrec = 1;
    long long N = 0;
    size_t budget = 0, resident = 0;
    long long row_blocks = 0;
    char *d = nullptr, *d_pair = nullptr;
    TcTrees dev{};
    std::vector<int> off, cnt, nreal, distinct;      // distinct: [T][2]
    std::vector<double> ss;                          // [T][2]: sums of squares of the normalised and of the raw lengths
    std::vector<int> ids, flags;                     // as the device left them (the doors)
    ~TreeCmp() { if (d_pair) hipFree(d_pair); if (d) hipFree(d); }

    // records, ids, sorted ids, per-tree sums and counts: everything but the pairs
    int prepare(int ntrees, const char *const *newicks, int use_lengths, bool keep_records) {
        std::string err;
        if (int rc = tc_build(ntrees, newicks, use_lengths, S, err)) return ctx->fail(rc, err);
        T = ntrees;
        const int W = S.W;
        off.resize((size_t)T + 1); cnt.resize((size_t)T); nreal.resize((size_t)T);
        for (int t = 0; t < T; ++t) {
            off[(size_t)t] = (int)N; cnt[(size_t)t] = S.trees[(size_t)t].nrec(); nreal[(size_t)t] = S.trees[(size_t)t].nreal;
            N += cnt[(size_t)t]; maxrec = std::max(maxrec, cnt[(size_t)t]);
            if (N > (1ll << 30)) return ctx->fail(PML_ENOMEM, "the trees have more than 2^30 split records together");
        }
        off[(size_t)T] = (int)N;
        if (maxrec > TC_SORT) return ctx->fail(PML_EINVAL, "a tree with " + std::to_string(maxrec) + " records");      // cannot happen: < 3 n
        const unsigned long long cap = pow2_at_least(2ull * (unsigned long long)N);
        size_t at = 0;
        auto take = [&](size_t bytes) { const size_t o = at; at += align_up(bytes, 256); return o; };
        const size_t o_rec = take((size_t)N * W * 8), o_ln = take((size_t)N * 8), o_lr = take((size_t)N * 8), o_ss = take((size_t)T * 16);
        const size_t o_off = take((size_t)(T + 1) * 4), o_cnt = take((size_t)T * 4), o_nreal = take((size_t)T * 4), o_flags = take((size_t)N * 4);
        const size_t up_bytes = at;                                  // everything above is uploaded in one copy
        const size_t o_id = take((size_t)N * 4), o_sid = take((size_t)N * 4), o_sidx = take((size_t)N * 4), o_dist = take((size_t)T * 8);
        const size_t o_count = take((size_t)N * 4), o_err = take(4), o_slot = take((size_t)cap * 4), o_first = take((size_t)N * 4);
        resident = at;
        TCCHK(hipSetDevice(ctx->device));
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = (size_t)1 << 40;
        budget = (size_t)(0.85 * (double)free_b);
        if (const char *e = std::getenv("PML_HBM_BUDGET_MB")) budget = (size_t)(std::max(0.0, std::strtod(e, nullptr)) * 1048576.0);
        if (resident > budget)
            return ctx->fail(PML_ENOMEM, "a tree comparison keeps the trees' records resident: " + std::to_string(N) + " records of " + std::to_string(T) + " trees need " +
                                             std::to_string(resident) + " bytes of HBM, the budget is " + std::to_string(budget) + " bytes");
        TCCHK(hipMalloc((void **)&d, resident));
        std::vector<char> host(up_bytes, 0);
        for (int t = 0; t < T; ++t) {
            const TcTree &tr = S.trees[(size_t)t];
            const size_t o = (size_t)off[(size_t)t], c = (size_t)cnt[(size_t)t];
            if (!c) continue;
            std::memcpy(host.data() + o_rec + o * W * 8, tr.words.data(), c * W * 8);
            std::memcpy(host.data() + o_ln + o * 8, tr.lnorm.data(), c * 8);
            std::memcpy(host.data() + o_lr + o * 8, tr.len.data(), c * 8);
            std::memcpy(host.data() + o_flags + o * 4, tr.flags.data(), c * 4);
        }
        std::memcpy(host.data() + o_off, off.data(), (size_t)(T + 1) * 4);
        std::memcpy(host.data() + o_cnt, cnt.data(), (size_t)T * 4);
        std::memcpy(host.data() + o_nreal, nreal.data(), (size_t)T * 4);
        TCCHK(hipMemcpyAsync(d, host.data(), up_bytes, hipMemcpyHostToDevice, ctx->stream));
        TCCHK(hipMemsetAsync(d + o_count, 0, o_slot - o_count, ctx->stream));                      // count, err
        TCCHK(hipMemsetAsync(d + o_slot, 0xFF, o_first - o_slot, ctx->stream));                    // slot = -1
        TCCHK(hipMemsetAsync(d + o_first, 0x7F, resident - o_first, ctx->stream));                 // first = 0x7F7F7F7F > 2^30
        dev = TcTrees{(const int *)(d + o_off), (const int *)(d + o_cnt), (const int *)(d + o_nreal), (int *)(d + o_id), (int *)(d + o_flags),
                      (const double *)(d + o_ln), (const double *)(d + o_lr), (int *)(d + o_sid), (int *)(d + o_sidx), T};
        launch_split_intern((const unsigned long long *)(d + o_rec), N, W, (int *)(d + o_slot), cap, ~0ull, dev.id, (int *)(d + o_count), (int *)(d + o_err), ctx->stream);
        launch_tree_first(dev.id, N, (int *)(d + o_first), ctx->stream);
        launch_tree_sort(dev, (double *)(d + o_ss), (int *)(d + o_dist), ctx->stream);
        TCCHK(hipGetLastError());
        ss.resize((size_t)T * 2); distinct.resize((size_t)T * 2);
        int bad = 0;
        TCCHK(hipMemcpyAsync(ss.data(), d + o_ss, (size_t)T * 16, hipMemcpyDeviceToHost, ctx->stream));
        TCCHK(hipMemcpyAsync(distinct.data(), d + o_dist, (size_t)T * 8, hipMemcpyDeviceToHost, ctx->stream));
        TCCHK(hipMemcpyAsync(&bad, d + o_err, 4, hipMemcpyDeviceToHost, ctx->stream));
        if (keep_records) {
            ids.resize((size_t)N); flags.resize((size_t)N);
            TCCHK(hipMemcpyAsync(ids.data(), dev.id, (size_t)N * 4, hipMemcpyDeviceToHost, ctx->stream));
            TCCHK(hipMemcpyAsync(flags.data(), dev.flags, (size_t)N * 4, hipMemcpyDeviceToHost, ctx->stream));
        }
        if (ctx->sync(ctx->stream)) return PML_EDEVICE;            // also: the staging vector goes out of scope
        if (bad) return ctx->fail(PML_EDEVICE, "the split table overflowed (a probe ran through all " + std::to_string(cap) + " slots)");
        return PML_OK;
    }

    // rows [r0, r1) against their columns j >= i; sink(i, counts of row i, sums of row i), entries j < i or outside the window unwritten
    template <class Sink>
    int pairs(int r0, int r1, int window, Sink &&sink) {
        const size_t row_bytes = (size_t)T * (sizeof(int4) + sizeof(double2));
        const size_t room = budget - resident;
        long long R = std::min<long long>({(long long)(room / row_bytes), (long long)(r1 - r0), (long long)TC_MAX_ROWS});
        if (R > 1) R = std::min<long long>(R, std::max<long long>(1, (long long)(TC_MAX_BLOCK_BYTES / row_bytes)));      // the host holds a copy of a block
        if (R < 1)
            return ctx->fail(PML_ENOMEM, "one row of pair outputs (" + std::to_string(T) + " trees, " + std::to_string(row_bytes) + " bytes) does not fit beside the " +
                                             std::to_string(resident) + " bytes of records: the budget is " + std::to_string(budget) + " bytes");
        TCCHK(hipMalloc((void **)&d_pair, (size_t)R * row_bytes));
        int4 *d_counts = (int4 *)d_pair;
        double2 *d_sums = (double2 *)(d_pair + (size_t)R * T * sizeof(int4));
        std::vector<int4> counts((size_t)R * T);
        std::vector<double2> sums((size_t)R * T);
        std::vector<double> nreal_prefix((size_t)T + 1, 0.0);
        for (int t = 0; t < T; ++t) nreal_prefix[(size_t)t + 1] = nreal_prefix[(size_t)t] + nreal[(size_t)t];
        for (int i0 = r0; i0 < r1; i0 += (int)R) {
            const int rows = (int)std::min<long long>(R, r1 - i0);
            double lookups = 0;                                      // set look-ups of the block: loop 1 over i's records, loop 2 over j's branches
            for (int i = i0; i < i0 + rows; ++i) {
                const int jend = window > 0 ? std::min(T, i + window + 1) : T;
                lookups += (double)cnt[(size_t)i] * (jend - i) + nreal_prefix[(size_t)jend] - nreal_prefix[(size_t)i];
            }
            ctx->tic(K_TREEPAIRS, 4.0 * lookups);
            launch_tree_pairs(dev, i0, rows, window, maxrec, d_counts, d_sums, ctx->stream);
            ctx->toc();
            TCCHK(hipGetLastError());
            TCCHK(hipMemcpyAsync(counts.data(), d_counts, (size_t)rows * T * sizeof(int4), hipMemcpyDeviceToHost, ctx->stream));
            TCCHK(hipMemcpyAsync(sums.data(), d_sums, (size_t)rows * T * sizeof(double2), hipMemcpyDeviceToHost, ctx->stream));
            if (ctx->sync(ctx->stream)) return PML_EDEVICE;
            ctx->resolve_events();
            ++row_blocks;
            for (int r = 0; r < rows; ++r) sink(i0 + r, counts.data() + (size_t)r * T, sums.data() + (size_t)r * T);
        }
        return PML_OK;
    }
};

struct Finish { int rf_legacy, rf_bipartition, rf_splits; double branch, discrepant; };
Finish finish(const TreeCmp &tc, int i, int j, const int4 &c, const double2 &s) {
    const int *di = tc.distinct.data() + 2 * (size_t)i, *dj = tc.distinct.data() + 2 * (size_t)j;
    const double *si = tc.ss.data() + 2 * (size_t)i, *sj = tc.ss.data() + 2 * (size_t)j;
    const long long inner = tc.S.n - 3;                           // inner edges of a resolved tree
    return Finish{tc_rf(di[0], dj[0], c.x), tc_rf(di[1], dj[1], c.y), tc_rf(inner, inner, c.z), tc_distance(s.x, si[0], sj[0]), tc_distance(s.y, si[1], sj[1])};
}

int want_of(const pml_tree_compare_opts *o) { return o && o->want ? o->want : 31; }

// rows x cols outputs; one: row 0 of a set whose tree 0 is the standard tree, columns 1 .. T - 1
int run(pml_ctx *pctx, int ntrees, const char *const *newicks, const pml_tree_compare_opts *opts, bool one, pml_tree_compare_result *out) {
    pml_fpguard fpg;
    pml_drop_worker_caches(pctx);
    Ctx *ctx = &pctx->c;
    try {
        const int window = one || !opts ? 0 : opts->window;
        if (window < 0) return ctx->fail(PML_EINVAL, "window must not be negative");
        TreeCmp tc; tc.ctx = ctx;
        if (int rc = tc.prepare(ntrees, newicks, opts ? opts->use_lengths : 1, false)) return rc;
        const int T = tc.T, want = want_of(opts);
        const size_t rows = one ? 1 : (size_t)T, cols = one ? (size_t)T - 1 : (size_t)T, cells = std::max<size_t>(rows * cols, 1);
        out->nrows = (int)rows; out->ncols = (int)cols; out->ntax = tc.S.n;
        if (want & PML_TC_RF_LEGACY) out->rf_legacy = (int *)std::malloc(cells * sizeof(int));
        if (want & PML_TC_RF_BIPARTITION) out->rf_bipartition = (int *)std::malloc(cells * sizeof(int));
        if (want & PML_TC_RF_SPLITS) out->rf_splits = (int *)std::malloc(cells * sizeof(int));
        if (want & PML_TC_BRANCH_DIST) out->branch_dist = (double *)std::malloc(cells * sizeof(double));
        if (want & PML_TC_DISCREPANT_DIST) out->discrepant_dist = (double *)std::malloc(cells * sizeof(double));
        if (((want & PML_TC_RF_LEGACY) && !out->rf_legacy) || ((want & PML_TC_RF_BIPARTITION) && !out->rf_bipartition) || ((want & PML_TC_RF_SPLITS) && !out->rf_splits) ||
            ((want & PML_TC_BRANCH_DIST) && !out->branch_dist) || ((want & PML_TC_DISCREPANT_DIST) && !out->discrepant_dist)) {
            pml_tree_compare_result_free(out); return ctx->fail(PML_ENOMEM, "host allocation failed");
        }
        const double nan = std::numeric_limits<double>::quiet_NaN();
        for (size_t k = 0; k < rows * cols; ++k) {                   // what a pair outside the window holds
            if (out->rf_legacy) out->rf_legacy[k] = -1;
            if (out->rf_bipartition) out->rf_bipartition[k] = -1;
            if (out->rf_splits) out->rf_splits[k] = -1;
            if (out->branch_dist) out->branch_dist[k] = nan;
            if (out->discrepant_dist) out->discrepant_dist[k] = nan;
        }
        auto put = [&](size_t k, const Finish &f) {
            if (out->rf_legacy) out->rf_legacy[k] = f.rf_legacy;
            if (out->rf_bipartition) out->rf_bipartition[k] = f.rf_bipartition;
            if (out->rf_splits) out->rf_splits[k] = f.rf_splits;
            if (out->branch_dist) out->branch_dist[k] = f.branch;
            if (out->discrepant_dist) out->discrepant_dist[k] = f.discrepant;
        };
        int rc = tc.pairs(0, one ? 1 : T, window, [&](int i, const int4 *c, const double2 *s) {
            const int jend = window > 0 ? std::min(T, i + window + 1) : T;
            for (int j = one ? 1 : i; j < jend; ++j) {
                Finish f = finish(tc, i, j, c[j], s[j]);
                if (one) { put((size_t)j - 1, f); continue; }
                if (i == j) f.rf_legacy = f.rf_bipartition = f.rf_splits = 0;
                put((size_t)i * T + j, f);
                put((size_t)j * T + i, f);                           // compareAllvsAll :274-275: [j][i] is a copy
            }
        });
        out->row_blocks = tc.row_blocks; out->resident_bytes = (long long)tc.resident; out->row_bytes = (long long)T * (long long)(sizeof(int4) + sizeof(double2));
        if (rc) { pml_tree_compare_result_free(out); return rc; }
        return PML_OK;
    } catch (const std::bad_alloc &) { pml_tree_compare_result_free(out); return ctx->fail(PML_ENOMEM, "host allocation failed"); }
    catch (const std::exception &e) { pml_tree_compare_result_free(out); return ctx->fail(PML_EINVAL, e.what()); }
}
}  // namespace

extern "C" void pml_tree_compare_result_free(pml_tree_compare_result *r) {
    if (!r) return;
    std::free(r->rf_legacy); std::free(r->rf_bipartition); std::free(r->rf_splits); std::free(r->branch_dist); std::free(r->discrepant_dist);
    std::memset(r, 0, sizeof *r);
}

extern "C" int pml_tree_compare(pml_ctx *ctx, int ntrees, const char *const *newicks, const pml_tree_compare_opts *opts, pml_tree_compare_result *out) {
    if (out) std::memset(out, 0, sizeof *out);
    if (!ctx || !out) return PML_EINVAL;
    std::lock_guard<std::mutex> lk(ctx->c.mu);
    if (ntrees < 1 || !newicks) return ctx->c.fail(PML_EINVAL, "a tree comparison needs at least one tree (" + std::to_string(ntrees) + " given)");
    return run(ctx, ntrees, newicks, opts, false, out);
}

extern "C" int pml_tree_compare_one(pml_ctx *ctx, const char *standard_newick, int ntrees, const char *const *newicks, const pml_tree_compare_opts *opts,
                                    pml_tree_compare_result *out) {
    if (out) std::memset(out, 0, sizeof *out);
    if (!ctx || !out) return PML_EINVAL;
    std::lock_guard<std::mutex> lk(ctx->c.mu);
    if (ntrees < 1 || !newicks || !standard_newick) return ctx->c.fail(PML_EINVAL, "a comparison against a standard tree needs the standard tree and at least one other tree");
    std::vector<const char *> all{standard_newick};
    all.insert(all.end(), newicks, newicks + ntrees);
    return run(ctx, ntrees + 1, all.data(), opts, true, out);
}

extern "C" void pml_tree_splits_free(pml_tree_splits *r) {
    if (!r) return;
    if (r->names) { for (int i = 0; i < r->ntax; ++i) std::free(r->names[i]); std::free(r->names); }
    std::free(r->first); std::free(r->nreal); std::free(r->split_words); std::free(r->length); std::free(r->length_norm); std::free(r->flags); std::free(r->split_id);
    std::memset(r, 0, sizeof *r);
}

extern "C" int pml_debug_tree_splits(pml_ctx *pctx, int ntrees, const char *const *newicks, int use_lengths, pml_tree_splits *out) {
    if (out) std::memset(out, 0, sizeof *out);
    if (!pctx || !out) return PML_EINVAL;
    std::lock_guard<std::mutex> lk(pctx->c.mu);
    Ctx *ctx = &pctx->c;
    if (ntrees < 1 || !newicks) return ctx->fail(PML_EINVAL, "a tree comparison needs at least one tree");
    pml_fpguard fpg;
    pml_drop_worker_caches(pctx);
    try {
        TreeCmp tc; tc.ctx = ctx;
        if (int rc = tc.prepare(ntrees, newicks, use_lengths, true)) return rc;
        const int n = tc.S.n, W = tc.S.W, T = tc.T; const size_t N = (size_t)tc.N, N1 = std::max<size_t>(N, 1);
        out->ntrees = T; out->ntax = n; out->words = W; out->nrecords = tc.N;
        out->names = (char **)std::calloc((size_t)n + 1, sizeof(char *));
        out->first = (long long *)std::malloc(((size_t)T + 1) * sizeof(long long)); out->nreal = (int *)std::malloc((size_t)T * sizeof(int));
        out->split_words = (unsigned long long *)std::malloc(N1 * W * 8); out->length = (double *)std::malloc(N1 * 8); out->length_norm = (double *)std::malloc(N1 * 8);
        out->flags = (int *)std::malloc(N1 * 4); out->split_id = (int *)std::malloc(N1 * 4);
        bool ok = out->names && out->first && out->nreal && out->split_words && out->length && out->length_norm && out->flags && out->split_id;
        for (int i = 0; ok && i < n; ++i) {
            const std::string &s = tc.S.names[(size_t)i];
            out->names[i] = (char *)std::malloc(s.size() + 1);
            if (out->names[i]) std::memcpy(out->names[i], s.c_str(), s.size() + 1); else ok = false;
        }
        if (!ok) { pml_tree_splits_free(out); return ctx->fail(PML_ENOMEM, "host allocation failed"); }
        for (int t = 0; t <= T; ++t) out->first[t] = tc.off[(size_t)t];
        for (int t = 0; t < T; ++t) {
            const TcTree &tr = tc.S.trees[(size_t)t];
            const size_t o = (size_t)tc.off[(size_t)t], c = (size_t)tc.cnt[(size_t)t];
            out->nreal[t] = tr.nreal;
            if (!c) continue;
            std::memcpy(out->split_words + o * W, tr.words.data(), c * W * 8);
            std::memcpy(out->length + o, tr.len.data(), c * 8);
            std::memcpy(out->length_norm + o, tr.lnorm.data(), c * 8);
        }
        std::copy(tc.flags.begin(), tc.flags.end(), out->flags);
        std::copy(tc.ids.begin(), tc.ids.end(), out->split_id);
        return PML_OK;
    } catch (const std::bad_alloc &) { pml_tree_splits_free(out); return ctx->fail(PML_ENOMEM, "host allocation failed"); }
    catch (const std::exception &e) { pml_tree_splits_free(out); return ctx->fail(PML_EINVAL, e.what()); }
}

extern "C" int pml_debug_tree_pair_sums(pml_ctx *pctx, int ntrees, const char *const *newicks, int use_lengths, int npairs, const int *pairs, long long *counts_out,
                                        double *sums_out) {
    if (!pctx) return PML_EINVAL;
    std::lock_guard<std::mutex> lk(pctx->c.mu);
    Ctx *ctx = &pctx->c;
    if (ntrees < 1 || !newicks || npairs < 0 || (npairs > 0 && (!pairs || !counts_out || !sums_out))) return ctx->fail(PML_EINVAL, "bad arguments");
    for (int p = 0; p < npairs; ++p)
        if (pairs[2 * p] < 0 || pairs[2 * p] > pairs[2 * p + 1] || pairs[2 * p + 1] >= ntrees)
            return ctx->fail(PML_EINVAL, "pair " + std::to_string(p) + ": 0 <= i <= j < ntrees is required (tree 1 of the Java is i)");
    pml_fpguard fpg;
    pml_drop_worker_caches(pctx);
    try {
        TreeCmp tc; tc.ctx = ctx;
        if (int rc = tc.prepare(ntrees, newicks, use_lengths, false)) return rc;
        std::vector<std::vector<int>> of_row((size_t)ntrees);
        for (int p = 0; p < npairs; ++p) of_row[(size_t)pairs[2 * p]].push_back(p);
        return tc.pairs(0, ntrees, 0, [&](int i, const int4 *c, const double2 *s) {
            for (int p : of_row[(size_t)i]) {
                const int j = pairs[2 * p + 1];
                long long *co = counts_out + 7 * (size_t)p; double *so = sums_out + 6 * (size_t)p;
                co[0] = c[j].x; co[1] = c[j].y; co[2] = c[j].z;
                co[3] = tc.distinct[2 * (size_t)i]; co[4] = tc.distinct[2 * (size_t)i + 1]; co[5] = tc.distinct[2 * (size_t)j]; co[6] = tc.distinct[2 * (size_t)j + 1];
                so[0] = s[j].x; so[1] = tc.ss[2 * (size_t)i]; so[2] = tc.ss[2 * (size_t)j];
                so[3] = s[j].y; so[4] = tc.ss[2 * (size_t)i + 1]; so[5] = tc.ss[2 * (size_t)j + 1];
            }
        });
    } catch (const std::bad_alloc &) { return ctx->fail(PML_ENOMEM, "host allocation failed"); }
    catch (const std::exception &e) { return ctx->fail(PML_EINVAL, e.what()); }
}
