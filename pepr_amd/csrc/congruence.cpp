// congruence.cpp -- the device-backed half of the congruence filter's C ABI (include/peprml.h): pml_congruence_costs,
// pml_congruence_filter, pml_debug_column_splits.  The kernels are congruence.hip, the two host rules congruence_host.cpp.
// A call is resident: the genes' bytes, one record per split of every column and the two hash tables live in HBM until it
// returns; a call that does not fit the budget is refused before anything of that stage is allocated.
#include <algorithm>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <set>
#include <unordered_map>

#include "../../include/peprml.h"
#include "api_types.hpp"
#include "congruence.hpp"
#include "congruence_dev.hpp"

using namespace pml;

namespace {
#define CGCHK(expr)                                                                                                   \
    do { hipError_t e_ = (expr);                                                                                      \
         if (e_ != hipSuccess) return ctx->fail(PML_EDEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); } while (0)

unsigned long long pow2_at_least(unsigned long long x) { unsigned long long c = 64; while (c < x) c <<= 1; return c; }

struct Congruence {
    Ctx *ctx = nullptr;
    std::vector<std::string> names; int n = 0, W = 1, ngenes = 0;
    std::vector<int> ncols;
    std::vector<std::vector<std::pair<int, int>>> order;     // per gene: (union index, row) ascending
    std::vector<char> host;                                  // stage 1's staging block, until the first sync
    long long total_cols = 0, nrec = 0;
    size_t budget = 0, used = 0;
    char *d_in = nullptr, *d_rec = nullptr, *d_k = nullptr;
    // stage 1 (d_in): genes | tile_gene | tile_first | maps and bytes | nsplit | rec_off
    size_t o_tiles = 0, o_first = 0, o_nsplit = 0, o_off = 0; int ntiles = 0, max_ntax = 0; double cells = 0;
    // stage 2 (d_rec): rec | rec_col | rec_gene | split_id | count | cost_rec | slot | keys | cost_sum | ndistinct | err
    size_t o_col = 0, o_gene = 0, o_id = 0, o_count = 0, o_costrec = 0, o_slot = 0, o_keys = 0, o_sum = 0, o_nd = 0, o_err = 0;
    unsigned long long cap = 0;
    ~Congruence() { if (d_k) hipFree(d_k); if (d_rec) hipFree(d_rec); if (d_in) hipFree(d_in); }

    int fits(size_t bytes, const char *what) {
        if (used + bytes > budget)
            return ctx->fail(PML_ENOMEM, std::string("the congruence filter keeps a call resident: ") + what + " need " + std::to_string((used + bytes + ((size_t)1 << 20) - 1) >> 20) +
                                             " MiB of HBM, the budget is " + std::to_string(budget >> 20) + " MiB (" + std::to_string(total_cols) + " columns, " +
                                             std::to_string(nrec) + " split records)");
        used += bytes;
        return PML_OK;
    }

    // the checks of the genes, the union (given: the one to use, the debug hook; else the genes' own) and every gene's rows in
    // ascending union index; a repeated name: its last row, as pml_concatenate
    int plan(int ng, const pml_alignment *genes, const std::vector<std::string> *given) {
        ngenes = ng;
        for (int g = 0; g < ng; ++g) {
            const pml_alignment &A = genes[g];
            if (!A.names || !A.rows || A.ntax <= 0) return ctx->fail(PML_EINVAL, "bad alignment (gene " + std::to_string(g) + ")");
            for (int i = 0; i < A.ntax; ++i) if (!A.names[i] || !A.rows[i]) return ctx->fail(PML_EINVAL, "bad alignment (gene " + std::to_string(g) + ")");
            if (A.nsites <= 0) return ctx->fail(PML_EPARSE, "gene " + std::to_string(g) + " has no columns (the reference drops such a gene from one of two arrays it indexes together)");
        }
        if (given) names = *given;
        else {
            std::set<std::string> uni;                     // std::set order == Arrays.sort for ASCII names (MSAConcatenator)
            for (int g = 0; g < ng; ++g) for (int i = 0; i < genes[g].ntax; ++i) uni.insert(genes[g].names[i]);
            names.assign(uni.begin(), uni.end());
        }
        n = (int)names.size();
        if (names.size() > (size_t)CG_MAX_TAXA)
            return ctx->fail(PML_EINVAL, "the genes have " + std::to_string(names.size()) + " taxa together: the congruence filter takes at most " + std::to_string(CG_MAX_TAXA));
        W = cg_words(n);
        std::unordered_map<std::string, int> index;
        for (int i = 0; i < n; ++i) index[names[i]] = i;
        order.assign((size_t)ng, {});
        for (int g = 0; g < ng; ++g) {
            std::vector<int> row_of((size_t)n, -1);
            for (int i = 0; i < genes[g].ntax; ++i) {
                auto it = index.find(genes[g].names[i]);
                if (it == index.end()) return ctx->fail(PML_EINVAL, std::string("taxon '") + genes[g].names[i] + "' is not in the union");
                if ((int)strnlen(genes[g].rows[i], (size_t)genes[g].nsites) < genes[g].nsites)
                    return ctx->fail(PML_EINVAL, "row shorter than nsites (gene " + std::to_string(g) + ", taxon '" + genes[g].names[i] + "')");
                row_of[(size_t)it->second] = i;
            }
            for (int u = 0; u < n; ++u) if (row_of[(size_t)u] >= 0) order[(size_t)g].push_back({u, row_of[(size_t)u]});
        }
        return PML_OK;
    }

    // stage 1 in HBM.  genes: their text is uploaded in the CgGene layout; resident: they are there already (col_base is set here)
    int stage(const pml_alignment *genes, const CgGene *resident) {
        const int ng = ngenes;
        std::vector<size_t> o_map((size_t)ng), o_bytes((size_t)ng), ld((size_t)ng);
        ncols.resize((size_t)ng);
        long long tiles = 0;
        for (int g = 0; g < ng; ++g) {
            ncols[g] = genes ? genes[g].nsites : resident[g].ncols; total_cols += ncols[g]; tiles += (ncols[g] + CG_COLS - 1) / CG_COLS;
            max_ntax = std::max(max_ntax, (int)order[(size_t)g].size());
            cells += (double)order[(size_t)g].size() * ncols[g];
        }
        if (tiles > INT_MAX) return ctx->fail(PML_EINVAL, "too many columns for one call");
        ntiles = (int)tiles;
        size_t off = align_up((size_t)ng * sizeof(CgGene), 256);
        o_tiles = off; off += align_up((size_t)ntiles * sizeof(int), 256);
        o_first = off; off += align_up((size_t)ng * sizeof(int), 256);
        for (int g = 0; genes && g < ng; ++g) {
            const size_t nt = order[(size_t)g].size();
            ld[g] = align_up((size_t)ncols[g], 16);
            o_map[g] = off; off += align_up(nt * sizeof(uint16_t), 256);
            o_bytes[g] = off; off += align_up(nt * ld[g], 256);
        }
        const size_t in_bytes = off;
        o_nsplit = off; off += align_up((size_t)total_cols * sizeof(int), 256);
        o_off = off; off += align_up((size_t)total_cols * sizeof(long long), 256);
        CGCHK(hipSetDevice(ctx->device));
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = (size_t)1 << 40;
        budget = (size_t)(0.85 * (double)free_b);
        if (const char *e = std::getenv("PML_HBM_BUDGET_MB")) budget = (size_t)std::atoll(e) << 20;
        else budget += used;                               // what a caller holds for this call was free before it took it
        if (int rc = fits(off, "the genes' bytes")) return rc;
        CGCHK(hipMalloc((void **)&d_in, off));
        host.assign(in_bytes, '?');
        {
            int *tile_gene = (int *)(host.data() + o_tiles), *tile_first = (int *)(host.data() + o_first);
            long long col_base = 0; int t = 0;
            for (int g = 0; g < ng; ++g) {
                const auto &ord = order[(size_t)g];
                if (genes) {
                    uint16_t *map = (uint16_t *)(host.data() + o_map[g]);
                    for (size_t r = 0; r < ord.size(); ++r) {
                        map[r] = (uint16_t)ord[r].first;
                        std::memcpy(host.data() + o_bytes[g] + r * ld[g], genes[g].rows[ord[r].second], (size_t)ncols[g]);
                    }
                    ((CgGene *)host.data())[g] = CgGene{(const uint8_t *)(d_in + o_bytes[g]), (const uint16_t *)(d_in + o_map[g]), (int)ord.size(), ncols[g], (int)ld[g], col_base};
                } else {
                    CgGene rg = resident[g]; rg.col_base = col_base;
                    ((CgGene *)host.data())[g] = rg;
                }
                tile_first[g] = t;
                for (int k = 0; k < (ncols[g] + CG_COLS - 1) / CG_COLS; ++k) tile_gene[t++] = g;
                col_base += ncols[g];
            }
        }
        CGCHK(hipMemcpyAsync(d_in, host.data(), in_bytes, hipMemcpyHostToDevice, ctx->stream));
        return PML_OK;
    }

    // rules 1 and 2: every column's splits as records in HBM
    int records() {
        const int ng = ngenes;
        ctx->tic(K_COLSPLIT, cells);
        launch_colsplits((const CgGene *)d_in, (const int *)(d_in + o_tiles), (const int *)(d_in + o_first), ntiles, max_ntax, n, (int *)(d_in + o_nsplit),
                         nullptr, nullptr, nullptr, nullptr, ctx->stream);
        ctx->toc();
        CGCHK(hipGetLastError());
        std::vector<int> nsplit((size_t)total_cols);
        CGCHK(hipMemcpyAsync(nsplit.data(), d_in + o_nsplit, nsplit.size() * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        if (ctx->sync(ctx->stream)) return PML_EDEVICE;
        ctx->resolve_events();
        std::vector<char>().swap(host);
        std::vector<long long> rec_off((size_t)total_cols);
        for (long long c = 0; c < total_cols; ++c) { rec_off[(size_t)c] = nrec; nrec += nsplit[(size_t)c]; }
        if (nrec > INT_MAX - 1) return ctx->fail(PML_ENOMEM, "the call has " + std::to_string(nrec) + " split records: at most 2^31 - 2 fit one call");
        if (nrec == 0) return PML_OK;
        cap = pow2_at_least(2ull * (unsigned long long)nrec);
        size_t off = 0;
        auto take = [&](size_t bytes) { const size_t at = off; off += align_up(bytes, 256); return at; };
        take((size_t)nrec * W * sizeof(unsigned long long));
        o_col = take((size_t)nrec * sizeof(long long)); o_gene = take((size_t)nrec * sizeof(int)); o_id = take((size_t)nrec * sizeof(int));
        o_count = take((size_t)nrec * sizeof(int)); o_costrec = take((size_t)nrec * sizeof(long long));
        o_slot = take((size_t)cap * sizeof(int)); o_keys = take((size_t)cap * sizeof(unsigned long long));
        o_sum = take((size_t)ng * sizeof(long long)); o_nd = take((size_t)ng * sizeof(int)); o_err = take(sizeof(int));
        if (int rc = fits(off, "the split records and their two hash tables")) return rc;
        CGCHK(hipMalloc((void **)&d_rec, off));
        CGCHK(hipMemcpyAsync(d_in + o_off, rec_off.data(), rec_off.size() * sizeof(long long), hipMemcpyHostToDevice, ctx->stream));
        CGCHK(hipMemsetAsync(d_rec + o_count, 0, o_slot - o_count, ctx->stream));                  // count, cost_rec
        CGCHK(hipMemsetAsync(d_rec + o_slot, 0xFF, o_sum - o_slot, ctx->stream));                  // slot = -1, keys = ~0
        CGCHK(hipMemsetAsync(d_rec + o_sum, 0, off - o_sum, ctx->stream));                         // cost_sum, ndistinct, err
        ctx->tic(K_COLSPLIT, cells);
        launch_colsplits((const CgGene *)d_in, (const int *)(d_in + o_tiles), (const int *)(d_in + o_first), ntiles, max_ntax, n, (int *)(d_in + o_nsplit),
                         (const long long *)(d_in + o_off), (unsigned long long *)d_rec, (int *)(d_rec + o_gene), (long long *)(d_rec + o_col), ctx->stream);
        ctx->toc();
        CGCHK(hipGetLastError());
        if (ctx->sync(ctx->stream)) return PML_EDEVICE;            // rec_off goes out of scope
        ctx->resolve_events();
        return PML_OK;
    }

    int extract(int ng, const pml_alignment *genes, const std::vector<std::string> *given) {
        if (int rc = plan(ng, genes, given)) return rc;
        if (int rc = stage(genes, nullptr)) return rc;
        return records();
    }

    // rules 3 to 6 on the records of extract()
    int charge(unsigned long long hash_mask, pml_congruence_result *res) {
        std::vector<long long> cost_sum((size_t)ngenes, 0); std::vector<int> ndist_g((size_t)ngenes, 0);
        std::vector<unsigned long long> kwords; std::vector<int> kcount; std::vector<long long> kcost;
        int cutoff = 0; size_t D = 0;
        if (nrec > 0) {
            const unsigned long long *rec = (const unsigned long long *)d_rec;
            int *split_id = (int *)(d_rec + o_id), *count = (int *)(d_rec + o_count), *err = (int *)(d_rec + o_err);
            launch_split_intern(rec, nrec, W, (int *)(d_rec + o_slot), cap, hash_mask, split_id, count, err, ctx->stream);
            CGCHK(hipGetLastError());
            std::vector<int> ids((size_t)nrec), counts((size_t)nrec); int bad = 0;
            CGCHK(hipMemcpyAsync(ids.data(), split_id, ids.size() * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
            CGCHK(hipMemcpyAsync(counts.data(), count, counts.size() * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
            CGCHK(hipMemcpyAsync(&bad, err, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
            if (ctx->sync(ctx->stream)) return PML_EDEVICE;
            if (bad) return ctx->fail(PML_EDEVICE, "the split table overflowed (a probe ran through all " + std::to_string(cap) + " slots)");
            // rule 4 on the owners' counts
            std::vector<int> dist, dcount;
            for (long long r = 0; r < nrec; ++r) if (ids[(size_t)r] == (int)r) { dist.push_back((int)r); dcount.push_back(counts[(size_t)r]); }
            D = dist.size();
            std::vector<size_t> kept;
            cutoff = cg_kept_set(dcount.data(), D, 4LL * n, kept);
            const size_t K = kept.size();
            std::vector<int> kidx(K); kcount.resize(K);
            for (size_t j = 0; j < K; ++j) { kidx[j] = dist[kept[j]]; kcount[j] = dcount[kept[j]]; }
            size_t off = 0;
            auto take = [&](size_t bytes) { const size_t at = off; off += align_up(bytes, 256); return at; };
            const size_t o_dist = take(D * sizeof(int)), o_kidx = take(K * sizeof(int)), o_kcount = take(K * sizeof(int));
            const size_t o_kw = take(K * W * sizeof(unsigned long long)), o_costd = take(D * sizeof(long long));
            if (int rc = fits(off, "the distinct and the kept splits")) return rc;
            CGCHK(hipMalloc((void **)&d_k, off));
            CGCHK(hipMemcpyAsync(d_k + o_dist, dist.data(), D * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
            if (K) {
                CGCHK(hipMemcpyAsync(d_k + o_kidx, kidx.data(), K * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
                CGCHK(hipMemcpyAsync(d_k + o_kcount, kcount.data(), K * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
            }
            launch_split_gather(rec, (const int *)(d_k + o_kidx), (long long)K, W, (unsigned long long *)(d_k + o_kw), ctx->stream);
            const double blocks = (double)((D + 255) / 256);
            ctx->tic(K_SPLITCOST, (double)D * W * 8 + blocks * (double)K * (W * 8 + 4));
            launch_splitcost(rec, (const int *)(d_k + o_dist), (long long)D, W, (const unsigned long long *)(d_k + o_kw), (const int *)(d_k + o_kcount), (long long)K,
                             (long long *)(d_k + o_costd), (long long *)(d_rec + o_costrec), ctx->stream);
            ctx->toc();
            launch_genecost((const int *)(d_rec + o_gene), split_id, nrec, (const long long *)(d_rec + o_costrec), (unsigned long long *)(d_rec + o_keys), cap,
                            hash_mask, (long long *)(d_rec + o_sum), (int *)(d_rec + o_nd), err, ctx->stream);
            CGCHK(hipGetLastError());
            std::vector<long long> cost_d(D); std::vector<unsigned long long> kw(K * W);
            CGCHK(hipMemcpyAsync(cost_d.data(), d_k + o_costd, D * sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
            if (K) CGCHK(hipMemcpyAsync(kw.data(), d_k + o_kw, kw.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
            CGCHK(hipMemcpyAsync(cost_sum.data(), d_rec + o_sum, cost_sum.size() * sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
            CGCHK(hipMemcpyAsync(ndist_g.data(), d_rec + o_nd, ndist_g.size() * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
            CGCHK(hipMemcpyAsync(&bad, err, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
            if (ctx->sync(ctx->stream)) return PML_EDEVICE;
            ctx->resolve_events();
            if (bad) return ctx->fail(PML_EDEVICE, "the gene table overflowed (a probe ran through all " + std::to_string(cap) + " slots)");
            // K ascending as n-bit integers, so that the output does not depend on which record came to own a split
            std::vector<size_t> by(K);
            for (size_t j = 0; j < K; ++j) by[j] = j;
            const int Wl = W;
            std::sort(by.begin(), by.end(), [&](size_t a, size_t b) {
                for (int w = Wl - 1; w >= 0; --w) if (kw[a * Wl + w] != kw[b * Wl + w]) return kw[a * Wl + w] < kw[b * Wl + w];
                return false; });
            std::vector<int> kc(K); kwords.resize(K * W); kcost.resize(K);
            for (size_t j = 0; j < K; ++j) {
                std::copy(kw.begin() + by[j] * W, kw.begin() + (by[j] + 1) * W, kwords.begin() + j * W);
                kc[j] = kcount[by[j]]; kcost[j] = cost_d[kept[by[j]]];
            }
            kcount.swap(kc);
        }
        // the result, library-owned
        const size_t K = kcount.size(), G = (size_t)ngenes;
        std::memset(res, 0, sizeof *res);
        res->ngenes = ngenes; res->ntax = n; res->words = W; res->cutoff = cutoff; res->nkept = (long long)K; res->nrecords = nrec; res->ndistinct = (long long)D;
        res->names = (char **)std::calloc((size_t)n + 1, sizeof(char *));
        res->cost_sum = (long long *)std::malloc(G * sizeof(long long)); res->mean_cost = (long long *)std::malloc(G * sizeof(long long));
        res->nsplits = (int *)std::malloc(G * sizeof(int));
        res->kept_words = (unsigned long long *)std::malloc(std::max<size_t>(K * W, 1) * sizeof(unsigned long long));
        res->kept_count = (long long *)std::malloc(std::max<size_t>(K, 1) * sizeof(long long)); res->kept_cost = (long long *)std::malloc(std::max<size_t>(K, 1) * sizeof(long long));
        bool ok = res->names && res->cost_sum && res->mean_cost && res->nsplits && res->kept_words && res->kept_count && res->kept_cost;
        for (int i = 0; ok && i < n; ++i) {
            res->names[i] = (char *)std::malloc(names[(size_t)i].size() + 1);
            if (res->names[i]) std::memcpy(res->names[i], names[(size_t)i].c_str(), names[(size_t)i].size() + 1); else ok = false;
        }
        if (!ok) { pml_congruence_result_free(res); return ctx->fail(PML_ENOMEM, "host allocation failed"); }
        for (size_t g = 0; g < G; ++g) { res->cost_sum[g] = cost_sum[g]; res->mean_cost[g] = cost_sum[g] / ncols[g]; res->nsplits[g] = ndist_g[g]; }
        std::copy(kwords.begin(), kwords.end(), res->kept_words);
        for (size_t j = 0; j < K; ++j) { res->kept_count[j] = kcount[j]; res->kept_cost[j] = kcost[j]; }
        return PML_OK;
    }
};

int costs_locked(pml_ctx *ctx, int ngenes, const pml_alignment *genes, const pml_congruence_opts *opts, pml_congruence_result *result) {
    pml_fpguard fpg;
    pml_drop_worker_caches(ctx);
    try {
        Congruence cg; cg.ctx = &ctx->c;
        if (int rc = cg.extract(ngenes, genes, nullptr)) return rc;
        return cg.charge(opts && opts->use_hash_mask ? opts->hash_mask : ~0ull, result);
    } catch (const std::bad_alloc &) { return ctx->c.fail(PML_ENOMEM, "host allocation failed"); }
    catch (const std::exception &e) { return ctx->c.fail(PML_EINVAL, e.what()); }
}
}  // namespace

int pml::cg_plan(Ctx *ctx, int ngenes, const pml_alignment *genes, CgPlan &plan) {
    Congruence cg; cg.ctx = ctx;
    if (int rc = cg.plan(ngenes, genes, nullptr)) return rc;
    plan.names.swap(cg.names); plan.order.swap(cg.order);
    return PML_OK;
}

int pml::cg_costs_resident(pml_ctx *ctx, const CgPlan &plan, const std::vector<CgGene> &genes, size_t resident_bytes, pml_congruence_result *result) {
    try {
        Congruence cg; cg.ctx = &ctx->c;
        cg.ngenes = (int)genes.size(); cg.names = plan.names; cg.n = (int)plan.names.size(); cg.W = cg_words(cg.n); cg.order = plan.order;
        cg.used = resident_bytes;
        for (size_t g = 0; g < genes.size(); ++g)
            if (genes[g].ncols <= 0) return ctx->c.fail(PML_EPARSE, "gene " + std::to_string(g) + " has no columns");
        if (int rc = cg.stage(nullptr, genes.data())) return rc;
        if (int rc = cg.records()) return rc;
        return cg.charge(~0ull, result);
    } catch (const std::bad_alloc &) { return ctx->c.fail(PML_ENOMEM, "host allocation failed"); }
    catch (const std::exception &e) { return ctx->c.fail(PML_EINVAL, e.what()); }
}

extern "C" void pml_congruence_result_free(pml_congruence_result *r) {
    if (!r) return;
    if (r->names) { for (int i = 0; i < r->ntax; ++i) std::free(r->names[i]); std::free(r->names); }
    std::free(r->cost_sum); std::free(r->mean_cost); std::free(r->nsplits); std::free(r->kept_words); std::free(r->kept_count); std::free(r->kept_cost);
    std::memset(r, 0, sizeof *r);
}

extern "C" int pml_congruence_costs(pml_ctx *ctx, int ngenes, const pml_alignment *genes, const pml_congruence_opts *opts, pml_congruence_result *result) {
    if (result) std::memset(result, 0, sizeof *result);
    if (!ctx || !genes || ngenes < 1 || !result) return PML_EINVAL;
    std::lock_guard<std::mutex> lk(ctx->c.mu);
    return costs_locked(ctx, ngenes, genes, opts, result);
}

extern "C" int pml_congruence_filter(pml_ctx *ctx, int ngenes, const pml_alignment *genes, double trim_percent, int *keep_out, pml_congruence_result *result) {
    if (result) std::memset(result, 0, sizeof *result);
    if (!ctx || !genes || ngenes < 1 || !keep_out) return PML_EINVAL;
    std::lock_guard<std::mutex> lk(ctx->c.mu);
    if (!(trim_percent > 0)) return ctx->c.fail(PML_EINVAL, "trim_percent must be positive (the reference throws)");
    pml_congruence_result local;
    pml_congruence_result *res = result ? result : &local;
    if (int rc = costs_locked(ctx, ngenes, genes, nullptr, res)) return rc;
    int rc = pml_congruence_select(ngenes, res->mean_cost, trim_percent, keep_out, nullptr, nullptr);
    if (rc) { pml_congruence_result_free(res); return ctx->c.fail(rc, "trim_percent puts the percentile index outside the genes (the reference throws)"); }
    if (!result) pml_congruence_result_free(&local);
    return PML_OK;
}

extern "C" int pml_debug_column_splits(pml_ctx *ctx, const pml_alignment *gene, int nunion, const char *const *names_union, long long *nrec_out,
                                       int *words_out, unsigned long long **records_out) {
    if (records_out) *records_out = nullptr;
    if (!ctx || !gene || nunion < 1 || !names_union || !nrec_out || !words_out || !records_out) return PML_EINVAL;
    std::lock_guard<std::mutex> lk(ctx->c.mu);
    pml_fpguard fpg;
    pml_drop_worker_caches(ctx);
    try {
        std::vector<std::string> uni;
        for (int i = 0; i < nunion; ++i) { if (!names_union[i]) return ctx->c.fail(PML_EINVAL, "null name in the union"); uni.push_back(names_union[i]); }
        Congruence cg; cg.ctx = &ctx->c;
        if (int rc = cg.extract(1, gene, &uni)) return rc;
        const int W = cg.W; const size_t R = (size_t)cg.nrec;
        std::vector<unsigned long long> rec(R * W); std::vector<long long> col(R);
        if (R) {
            Ctx *c = &ctx->c;
            hipError_t e = hipMemcpy(rec.data(), cg.d_rec, rec.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost);
            if (e == hipSuccess) e = hipMemcpy(col.data(), cg.d_rec + cg.o_col, col.size() * sizeof(long long), hipMemcpyDeviceToHost);
            if (e != hipSuccess) return c->fail(PML_EDEVICE, std::string("reading the records back: ") + hipGetErrorString(e));
        }
        unsigned long long *out = (unsigned long long *)std::malloc(std::max<size_t>(R * (W + 1), 1) * sizeof(unsigned long long));
        if (!out) return ctx->c.fail(PML_ENOMEM, "host allocation failed");
        for (size_t r = 0; r < R; ++r) { out[r * (W + 1)] = (unsigned long long)col[r]; std::copy(rec.begin() + r * W, rec.begin() + (r + 1) * W, out + r * (W + 1) + 1); }
        *nrec_out = cg.nrec; *words_out = W; *records_out = out;
    } catch (const std::bad_alloc &) { return ctx->c.fail(PML_ENOMEM, "host allocation failed"); }
    catch (const std::exception &e) { return ctx->c.fail(PML_EINVAL, e.what()); }
    return PML_OK;
}

extern "C" int pml_congruence_ktile(void) { return CG_KTILE; }
