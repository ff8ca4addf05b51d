// trim.cpp -- the host half of column trimming (include/peprml.h): pml_trim_columns, pml_trim_congruence_filter,
// pml_trim_pipeline, pml_debug_column_flags, pml_trim_column_flags_host, pml_trim_stats.  The kernels are trim.hip, the rules trim.hpp.
// A sub-batch of genes is resident as ONE allocation: the genes in the CgGene layout (rows 16-byte padded), one flag byte per
// column, the kept columns' source indices and the trimmed matrices.  The host reads the flags back, builds every gene's kept
// columns as an exclusive prefix and uploads them, as the congruence path does with nsplit / rec_off; there is no device scan.
// pml_trim_pipeline puts the block trimmer's sub-batch (gblocks.cpp, trim_dev.hpp) in front: its trimmed matrices stay in HBM
// and this file's sub-batch classifies them where they are.
#include <algorithm>
#include <climits>
#include <cstdlib>
#include <cstring>

#include "../../include/peprml.h"
#include "api_types.hpp"
#include "congruence_dev.hpp"
#include "trim.hpp"
#include "trim_dev.hpp"

using namespace pml;

namespace pml {
int trim_check_gene(Ctx *ctx, const pml_alignment &A, int g) {
    if (!A.rows || A.ntax <= 0 || A.nsites < 0) return ctx->fail(PML_EINVAL, "bad alignment (gene " + std::to_string(g) + ")");
    for (int i = 0; i < A.ntax; ++i) {
        if (!A.rows[i]) return ctx->fail(PML_EINVAL, "bad alignment (gene " + std::to_string(g) + ")");
        if ((int)strnlen(A.rows[i], (size_t)A.nsites) < A.nsites)
            return ctx->fail(PML_EINVAL, "row shorter than nsites (gene " + std::to_string(g) + ", row " + std::to_string(i) + ")");
    }
    return PML_OK;
}

size_t trim_hbm_budget(Ctx *ctx) {
    hipSetDevice(ctx->device);
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = (size_t)1 << 40;
    size_t budget = (size_t)(0.85 * (double)free_b);
    if (const char *e = std::getenv("PML_HBM_BUDGET_MB")) budget = (size_t)std::atoll(e) << 20;
    return budget;
}

int trim_gather_tiles(int ntax, size_t ld_out) {
    return (int)((ld_out / 16 + TRIM_CHUNKS - 1) / TRIM_CHUNKS) * ((ntax + TRIM_ROWS - 1) / TRIM_ROWS);
}

int trim_result_alloc(pml_trim_result *res, int ngenes) {
    std::memset(res, 0, sizeof *res);
    res->ngenes = ngenes;
    const size_t G = (size_t)ngenes;
    res->ntax = (int *)std::calloc(G, sizeof(int)); res->ncols = (int *)std::calloc(G, sizeof(int)); res->nkept = (int *)std::calloc(G, sizeof(int));
    res->kept_cols = (int **)std::calloc(G, sizeof(int *)); res->rows = (char ***)std::calloc(G, sizeof(char **));
    res->gap_or_missing = (long long *)std::calloc(G, sizeof(long long));
    return res->ntax && res->ncols && res->nkept && res->kept_cols && res->rows && res->gap_or_missing ? PML_OK : PML_ENOMEM;
}

int trim_fill_gene(pml_trim_result *res, int g, int ntax, int ncols, long long gom, const std::vector<int> &kept, const std::vector<int> &rowsrc,
                   const char *rows, size_t ld_out) {
    const int nkept = (int)kept.size();
    res->ntax[g] = ntax; res->ncols[g] = ncols; res->nkept[g] = nkept; res->gap_or_missing[g] = gom;
    res->kept_cols[g] = (int *)std::malloc(std::max<size_t>((size_t)nkept, 1) * sizeof(int));
    res->rows[g] = (char **)std::calloc((size_t)ntax, sizeof(char *));
    if (!res->kept_cols[g] || !res->rows[g]) return PML_ENOMEM;
    std::copy(kept.begin(), kept.end(), res->kept_cols[g]);
    for (int p = 0; p < ntax; ++p) {
        char *row = (char *)std::malloc((size_t)nkept + 1);
        if (!row) return PML_ENOMEM;
        if (nkept) std::memcpy(row, rows + (size_t)p * ld_out, (size_t)nkept);
        row[nkept] = 0;
        res->rows[g][rowsrc[(size_t)p]] = row;
    }
    return PML_OK;
}
}  // namespace pml

namespace {
#define TRCHK(expr)                                                                                                   \
    do { hipError_t e_ = (expr);                                                                                      \
         if (e_ != hipSuccess) return ctx->fail(PML_EDEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); } while (0)

const unsigned KEEP_BIT[3] = {TRIM_KEEP_UNIFORM, TRIM_KEEP_GAP_UNIFORM, TRIM_KEEP_TOPOLOGICAL};

// what one gene adds to a sub-batch's allocation: input, output (at most the input's size), source columns, flags, map, tiles
// and descriptors, every per-gene array padded to 256 bytes
size_t gene_cost(int ntax, int ncols, bool with_map) {
    const size_t ld = align_up((size_t)ncols, 16);
    size_t b = 2 * align_up((size_t)ntax * ld, 256) + align_up(ld * sizeof(int), 256) + (size_t)ncols;
    if (with_map) b += align_up((size_t)ntax * sizeof(uint16_t), 256);
    b += sizeof(int) * (size_t)((ncols + TRIM_COLS - 1) / TRIM_COLS) + sizeof(TgTile) * (size_t)trim_gather_tiles(ntax, ld);
    return b + sizeof(CgGene) + sizeof(TgGene) + sizeof(long long) + sizeof(int);
}

struct TrimBatch {
    Ctx *ctx = nullptr;
    int ng = 0, first = 0;                         // genes first .. first + ng - 1 of the call
    std::vector<int> ntax, nmap, ncols, nkept;
    std::vector<std::vector<int>> rowsrc, kept;    // per gene: input row of every uploaded row; kept columns, ascending
    std::vector<size_t> ld, ld_out, o_bytes, o_map, o_out, o_src;
    std::vector<long long> gom;
    std::vector<uint8_t> flags;
    std::vector<char> host, out_host;
    long long total_cols = 0;
    size_t o_tiles = 0, o_first = 0, o_flags = 0, o_gom = 0, o_tg = 0, o_tt = 0, o_var = 0, bytes = 0, out0 = 0, out1 = 0;
    int ntiles = 0;
    char *d = nullptr;
    std::vector<const uint8_t *> in_ptr;           // per gene: its rows in HBM, here or in the stage before
    std::vector<const uint16_t *> map_ptr;
    ~TrimBatch() { if (d) hipFree(d); }

    // genes[first .. first + count): upload and k_colclass.  plan: rows in the plan's order (the chained call), with the map.
    // resident: the genes as the stage before left them in HBM, rows as resident_rows lists them; nothing is uploaded but the descriptors
    int classify(const pml_alignment *genes, int first_, int count, const CgPlan *plan, const std::vector<TrimResident> *resident = nullptr,
                 const std::vector<std::vector<int>> *resident_rows = nullptr) {
        first = first_; ng = count;
        ntax.resize(ng); nmap.assign(ng, 0); ncols.resize(ng); rowsrc.assign(ng, {}); ld.resize(ng); o_bytes.resize(ng); o_map.assign(ng, 0);
        in_ptr.assign(ng, nullptr); map_ptr.assign(ng, nullptr);
        long long tiles = 0; size_t bound = TRIM_BATCH_SLACK; int max_gt = 0;
        for (int i = 0; i < ng; ++i) {
            const pml_alignment &A = genes[first + i];
            ntax[i] = A.ntax; ncols[i] = resident ? (*resident)[(size_t)i].ncols : A.nsites;
            ld[i] = resident ? (*resident)[(size_t)i].ld : align_up((size_t)A.nsites, 16);
            total_cols += ncols[i]; tiles += (ncols[i] + TRIM_COLS - 1) / TRIM_COLS;
            bound += gene_cost(A.ntax, ncols[i], plan != nullptr);
            max_gt += trim_gather_tiles(A.ntax, ld[i]);
            std::vector<int> &rs = rowsrc[i];
            if (resident) { rs = (*resident_rows)[(size_t)i]; nmap[i] = (*resident)[(size_t)i].nmap; }
            else if (plan) {                            // the rows the congruence stage reads first, a repeated name's earlier rows behind them
                std::vector<char> taken((size_t)A.ntax, 0);
                for (auto &ur : plan->order[(size_t)(first + i)]) { rs.push_back(ur.second); taken[(size_t)ur.second] = 1; }
                nmap[i] = (int)rs.size();
                for (int r = 0; r < A.ntax; ++r) if (!taken[(size_t)r]) rs.push_back(r);
            } else for (int r = 0; r < A.ntax; ++r) rs.push_back(r);
        }
        if (tiles > INT_MAX) return ctx->fail(PML_EINVAL, "too many columns for one call");
        ntiles = (int)tiles;
        size_t off = align_up((size_t)ng * sizeof(CgGene), 256);
        o_tiles = off; off += align_up((size_t)ntiles * sizeof(int), 256);
        o_first = off; off += align_up((size_t)ng * sizeof(int), 256);
        for (int i = 0; i < ng && !resident; ++i) {
            if (plan) { o_map[i] = off; off += align_up((size_t)nmap[i] * sizeof(uint16_t), 256); }
            o_bytes[i] = off; off += align_up((size_t)ntax[i] * ld[i], 256);
        }
        const size_t in_bytes = off;
        o_flags = off; off += align_up((size_t)total_cols, 256);
        o_gom = off; off += align_up((size_t)ng * sizeof(long long), 256);
        o_tg = off; off += align_up((size_t)ng * sizeof(TgGene), 256);
        o_tt = off; off += align_up((size_t)max_gt * sizeof(TgTile), 256);
        o_var = off;                               // source columns and trimmed matrices, laid out once the flags are known
        bytes = std::max(bound, off);
        for (int i = 0; i < ng; ++i) off += align_up(ld[i] * sizeof(int), 256) + align_up((size_t)ntax[i] * ld[i], 256);
        if (resident) bytes = off;                 // the bound counts an input copy that is not here
        if (off > bytes) return ctx->fail(PML_EINVAL, "internal: a trim sub-batch outgrew its bound");
        TRCHK(hipSetDevice(ctx->device));
        TRCHK(hipMalloc((void **)&d, bytes));
        host.assign(in_bytes, 0);
        int *tile_gene = (int *)(host.data() + o_tiles), *tile_first = (int *)(host.data() + o_first);
        long long col_base = 0; int t = 0;
        for (int i = 0; i < ng; ++i) {
            const pml_alignment &A = genes[first + i];
            for (int p = 0; p < ntax[i] && !resident; ++p) std::memcpy(host.data() + o_bytes[i] + (size_t)p * ld[i], A.rows[rowsrc[i][(size_t)p]], (size_t)ncols[i]);
            if (plan && !resident) {
                uint16_t *map = (uint16_t *)(host.data() + o_map[i]);
                for (int p = 0; p < nmap[i]; ++p) map[p] = (uint16_t)plan->order[(size_t)(first + i)][(size_t)p].first;
            }
            in_ptr[i] = resident ? (*resident)[(size_t)i].bytes : (const uint8_t *)(d + o_bytes[i]);
            map_ptr[i] = resident ? (*resident)[(size_t)i].map : plan ? (const uint16_t *)(d + o_map[i]) : nullptr;
            ((CgGene *)host.data())[i] = CgGene{in_ptr[i], map_ptr[i], ntax[i], ncols[i], (int)ld[i], col_base};
            tile_first[i] = t;
            for (int k = 0; k < (ncols[i] + TRIM_COLS - 1) / TRIM_COLS; ++k) tile_gene[t++] = i;
            col_base += ncols[i];
        }
        hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
        if (ctx->profile) for (auto &e : ev) e = ctx->get_event();
        struct Back { Ctx *c; hipEvent_t *e; ~Back() { for (int k = 0; k < 3; ++k) if (e[k]) c->pool.push_back(e[k]); } } back{ctx, ev};
        if (ev[0]) hipEventRecord(ev[0], ctx->stream);
        TRCHK(hipMemcpyAsync(d, host.data(), in_bytes, hipMemcpyHostToDevice, ctx->stream));
        if (ev[1]) hipEventRecord(ev[1], ctx->stream);
        TRCHK(hipMemsetAsync(d + o_gom, 0, (size_t)ng * sizeof(long long), ctx->stream));
        launch_colclass((const CgGene *)d, (const int *)(d + o_tiles), (const int *)(d + o_first), ntiles, (uint8_t *)(d + o_flags), (long long *)(d + o_gom), ctx->stream);
        if (ev[2]) hipEventRecord(ev[2], ctx->stream);
        if (ntiles > 0) ctx->colclass_launches++;
        TRCHK(hipGetLastError());
        flags.resize((size_t)total_cols); gom.resize((size_t)ng);
        if (total_cols) TRCHK(hipMemcpyAsync(flags.data(), d + o_flags, flags.size(), hipMemcpyDeviceToHost, ctx->stream));
        TRCHK(hipMemcpyAsync(gom.data(), d + o_gom, gom.size() * sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
        if (ctx->sync(ctx->stream)) return PML_EDEVICE;
        if (ev[0]) {
            float ms = 0;
            if (hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) ctx->trim_ms[2] += ms;
            if (hipEventElapsedTime(&ms, ev[1], ev[2]) == hipSuccess) ctx->trim_ms[0] += ms;
        }
        std::vector<char>().swap(host);
        return PML_OK;
    }

    // the kept columns of every gene under `mode`, then k_colgather; download: the trimmed matrices come back to out_host
    int gather(int mode, bool download) {
        const unsigned bit = KEEP_BIT[mode];
        kept.assign(ng, {}); nkept.assign(ng, 0); ld_out.assign(ng, 0); o_out.assign(ng, 0); o_src.assign(ng, 0);
        size_t at = 0;
        for (int i = 0; i < ng; ++i) {
            const uint8_t *f = flags.data() + at; at += (size_t)ncols[i];
            for (int c = 0; c < ncols[i]; ++c) {
                if (mode == PML_TRIM_UNIFORM && (f[c] & TRIM_ALL_GAP))
                    return ctx->fail(PML_EPARSE, "gene " + std::to_string(first + i) + ", column " + std::to_string(c) +
                                                     " holds nothing but '-' and '?' (the reference's trimUniformColumns dereferences null there)");
                if (f[c] & bit) kept[i].push_back(c);
            }
            nkept[i] = (int)kept[i].size(); ld_out[i] = align_up((size_t)nkept[i], 16);
        }
        size_t off = o_var;
        for (int i = 0; i < ng; ++i) { o_src[i] = off; off += align_up(ld_out[i] * sizeof(int), 256); }
        const size_t src_bytes = off - o_var;
        out0 = off;
        for (int i = 0; i < ng; ++i) { o_out[i] = off; off += align_up((size_t)ntax[i] * ld_out[i], 256); }
        out1 = off;                                // <= bytes: ld_out <= ld, gene for gene
        std::vector<char> src_host(src_bytes, (char)0xFF);         // the padding entries: -1, never read as a column
        std::vector<TgGene> tg((size_t)ng); std::vector<TgTile> tt;
        for (int i = 0; i < ng; ++i) {
            if (nkept[i]) std::memcpy(src_host.data() + (o_src[i] - o_var), kept[i].data(), (size_t)nkept[i] * sizeof(int));
            tg[i] = TgGene{in_ptr[i], (uint8_t *)(d + o_out[i]), (const int *)(d + o_src[i]), ntax[i], nkept[i], (int)ld[i], (int)ld_out[i]};
            if (!nkept[i]) continue;               // no gather work
            for (int q = 0; q < (int)(ld_out[i] / 16); q += TRIM_CHUNKS)
                for (int r = 0; r < ntax[i]; r += TRIM_ROWS) tt.push_back(TgTile{i, q, r, 0});
        }
        hipEvent_t ev[2] = {nullptr, nullptr};
        if (ctx->profile) for (auto &e : ev) e = ctx->get_event();
        struct Back { Ctx *c; hipEvent_t *e; ~Back() { for (int k = 0; k < 2; ++k) if (e[k]) c->pool.push_back(e[k]); } } back{ctx, ev};
        if (!tt.empty()) {
            TRCHK(hipMemcpyAsync(d + o_var, src_host.data(), src_bytes, hipMemcpyHostToDevice, ctx->stream));
            TRCHK(hipMemcpyAsync(d + o_tg, tg.data(), tg.size() * sizeof(TgGene), hipMemcpyHostToDevice, ctx->stream));
            TRCHK(hipMemcpyAsync(d + o_tt, tt.data(), tt.size() * sizeof(TgTile), hipMemcpyHostToDevice, ctx->stream));
            if (ev[0]) hipEventRecord(ev[0], ctx->stream);
            launch_colgather((const TgGene *)(d + o_tg), (const TgTile *)(d + o_tt), (int)tt.size(), ctx->stream);
            if (ev[1]) hipEventRecord(ev[1], ctx->stream);
            ctx->colgather_launches++;
            TRCHK(hipGetLastError());
            if (download) {
                out_host.resize(out1 - out0);
                TRCHK(hipMemcpyAsync(out_host.data(), d + out0, out_host.size(), hipMemcpyDeviceToHost, ctx->stream));
            }
            if (ctx->sync(ctx->stream)) return PML_EDEVICE;        // the three staging vectors go out of scope
            if (ev[0]) { float ms = 0; if (hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) ctx->trim_ms[1] += ms; }
        }
        return PML_OK;
    }

    // genes first .. first + ng - 1 of the result, from out_host
    int fill(pml_trim_result *res) const {
        for (int i = 0; i < ng; ++i)
            if (trim_fill_gene(res, first + i, ntax[i], ncols[i], gom[i], kept[i], rowsrc[i], nkept[i] ? out_host.data() + (o_out[i] - out0) : nullptr, ld_out[i]))
                return PML_ENOMEM;
        return PML_OK;
    }
};

int trim_locked(pml_ctx *pctx, int ngenes, const pml_alignment *genes, int mode, pml_trim_result *result) {
    Ctx *ctx = &pctx->c;
    for (int g = 0; g < ngenes; ++g) if (int rc = trim_check_gene(ctx, genes[g], g)) return rc;
    const size_t budget = trim_hbm_budget(ctx);
    if (trim_result_alloc(result, ngenes)) return ctx->fail(PML_ENOMEM, "host allocation failed");
    for (int g0 = 0; g0 < ngenes;) {
        size_t need = TRIM_BATCH_SLACK; int g1 = g0;
        while (g1 < ngenes) {
            const size_t c = gene_cost(genes[g1].ntax, genes[g1].nsites, false);
            if (need + c > budget) break;
            need += c; ++g1;
        }
        if (g1 == g0) {
            const size_t c = TRIM_BATCH_SLACK + gene_cost(genes[g0].ntax, genes[g0].nsites, false);
            return ctx->fail(PML_ENOMEM, "gene " + std::to_string(g0) + " (" + std::to_string(genes[g0].ntax) + " rows, " + std::to_string(genes[g0].nsites) +
                                             " columns) needs " + std::to_string((c + ((size_t)1 << 20) - 1) >> 20) + " MiB of HBM for its bytes, flags and trimmed copy, the budget is " +
                                             std::to_string(budget >> 20) + " MiB");
        }
        TrimBatch tb; tb.ctx = ctx;
        if (int rc = tb.classify(genes, g0, g1 - g0, nullptr)) return rc;
        if (int rc = tb.gather(mode, true)) return rc;
        if (tb.fill(result)) return ctx->fail(PML_ENOMEM, "host allocation failed");
        g0 = g1;
    }
    return PML_OK;
}

// seen1 / seen2 / shown of every column on the host, through trim.hpp's functions
void host_flags(const pml_alignment &A, unsigned char *out) {
    for (int c = 0; c < A.nsites; ++c) {
        uint32_t seen1[8] = {0, 0, 0, 0, 0, 0, 0, 0}, seen2[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        int shown = 0;
        for (int r = 0; r < A.ntax; ++r) trim_note(seen1, seen2, shown, (unsigned char)A.rows[r][c]);
        out[c] = (unsigned char)trim_decide(seen1, seen2, shown, A.ntax);
    }
}
}  // namespace

extern "C" void pml_trim_result_free(pml_trim_result *r) {
    if (!r) return;
    for (int g = 0; g < r->ngenes; ++g) {
        if (r->kept_cols) std::free(r->kept_cols[g]);
        if (r->rows && r->rows[g]) { for (int i = 0; r->ntax && i < r->ntax[g]; ++i) std::free(r->rows[g][i]); std::free(r->rows[g]); }
    }
    std::free(r->ntax); std::free(r->ncols); std::free(r->nkept); std::free(r->kept_cols); std::free(r->rows); std::free(r->gap_or_missing);
    std::memset(r, 0, sizeof *r);
}

extern "C" int pml_trim_columns(pml_ctx *ctx, int ngenes, const pml_alignment *genes, int mode, pml_trim_result *result) {
    if (result) std::memset(result, 0, sizeof *result);
    if (!ctx || !genes || ngenes < 1 || !result) return PML_EINVAL;
    std::lock_guard<std::mutex> lk(ctx->c.mu);
    if (mode < PML_TRIM_UNIFORM || mode > PML_TRIM_TOPOLOGICAL) return ctx->c.fail(PML_EINVAL, "mode must be PML_TRIM_UNIFORM, PML_TRIM_GAP_UNIFORM or PML_TRIM_TOPOLOGICAL");
    pml_fpguard fpg;
    pml_drop_worker_caches(ctx);
    int rc;
    try { rc = trim_locked(ctx, ngenes, genes, mode, result); }
    catch (const std::bad_alloc &) { rc = ctx->c.fail(PML_ENOMEM, "host allocation failed"); }
    catch (const std::exception &e) { rc = ctx->c.fail(PML_EINVAL, e.what()); }
    if (rc) pml_trim_result_free(result);
    return rc;
}

extern "C" int pml_trim_congruence_filter(pml_ctx *pctx, int ngenes, const pml_alignment *genes, int mode, double trim_percent, int *keep_out,
                                          pml_trim_result *trim_result, pml_congruence_result *congruence_result) {
    if (trim_result) std::memset(trim_result, 0, sizeof *trim_result);
    if (congruence_result) std::memset(congruence_result, 0, sizeof *congruence_result);
    if (!pctx || !genes || ngenes < 1 || !keep_out) return PML_EINVAL;
    std::lock_guard<std::mutex> lk(pctx->c.mu);
    Ctx *ctx = &pctx->c;
    if (mode < PML_TRIM_UNIFORM || mode > PML_TRIM_TOPOLOGICAL) return ctx->fail(PML_EINVAL, "mode must be PML_TRIM_UNIFORM, PML_TRIM_GAP_UNIFORM or PML_TRIM_TOPOLOGICAL");
    if (!(trim_percent > 0)) return ctx->fail(PML_EINVAL, "trim_percent must be positive (the reference throws)");
    pml_fpguard fpg;
    pml_drop_worker_caches(pctx);
    pml_congruence_result local;
    pml_congruence_result *res = congruence_result ? congruence_result : &local;
    std::memset(res, 0, sizeof *res);
    int rc = PML_OK;
    try {
        CgPlan plan;
        if ((rc = cg_plan(ctx, ngenes, genes, plan))) return rc;
        size_t need = TRIM_BATCH_SLACK;
        for (int g = 0; g < ngenes; ++g) need += gene_cost(genes[g].ntax, genes[g].nsites, true);
        const size_t budget = trim_hbm_budget(ctx);
        if (need > budget)
            return ctx->fail(PML_ENOMEM, "the chained call keeps every gene resident: their bytes, flags and trimmed copies need " + std::to_string((need + ((size_t)1 << 20) - 1) >> 20) +
                                             " MiB of HBM, the budget is " + std::to_string(budget >> 20) + " MiB");
        TrimBatch tb; tb.ctx = ctx;
        if ((rc = tb.classify(genes, 0, ngenes, &plan))) return rc;
        if ((rc = tb.gather(mode, trim_result != nullptr))) return rc;
        std::vector<CgGene> resident((size_t)ngenes);
        for (int g = 0; g < ngenes; ++g) {
            if (tb.nkept[g] == 0)
                return ctx->fail(PML_EPARSE, "gene " + std::to_string(g) + " has no columns left after trimming (the reference divides by zero there)");
            // the trimmed matrix's first nmap rows are the plan's, in ascending union index, with the input's map
            resident[(size_t)g] = CgGene{(const uint8_t *)(tb.d + tb.o_out[g]), tb.map_ptr[(size_t)g], tb.nmap[g], tb.nkept[g], (int)tb.ld_out[g], 0};
        }
        if ((rc = cg_costs_resident(pctx, plan, resident, tb.bytes, res))) return rc;
        rc = pml_congruence_select(ngenes, res->mean_cost, trim_percent, keep_out, nullptr, nullptr);
        if (rc) { pml_congruence_result_free(res); return ctx->fail(rc, "trim_percent puts the percentile index outside the genes (the reference throws)"); }
        if (trim_result && (trim_result_alloc(trim_result, ngenes) || tb.fill(trim_result))) {
            pml_trim_result_free(trim_result); pml_congruence_result_free(res);
            return ctx->fail(PML_ENOMEM, "host allocation failed");
        }
    } catch (const std::bad_alloc &) { pml_congruence_result_free(res); if (trim_result) pml_trim_result_free(trim_result); return ctx->fail(PML_ENOMEM, "host allocation failed"); }
    catch (const std::exception &e) { pml_congruence_result_free(res); if (trim_result) pml_trim_result_free(trim_result); return ctx->fail(PML_EINVAL, e.what()); }
    if (!congruence_result) pml_congruence_result_free(&local);
    return PML_OK;
}

namespace {
int pipeline_locked(pml_ctx *pctx, int ngenes, const pml_alignment *genes, const pml_gblocks_params *gbp, bool use_gb, int mode, double trim_percent, int *keep_out,
                    pml_trim_result *gb_result, pml_trim_result *trim_result, pml_congruence_result *res) {
    Ctx *ctx = &pctx->c;
    const bool use_trim = mode >= 0, use_cg = trim_percent > 0;
    int rc;
    CgPlan plan;
    if (use_cg) { if ((rc = cg_plan(ctx, ngenes, genes, plan))) return rc; }
    else for (int g = 0; g < ngenes; ++g) if ((rc = trim_check_gene(ctx, genes[g], g))) return rc;
    size_t need = TRIM_BATCH_SLACK * 2;
    for (int g = 0; g < ngenes; ++g)
        need += (use_gb ? gb_gene_cost(genes[g].ntax, genes[g].nsites, use_cg) : 0) + (use_trim ? gene_cost(genes[g].ntax, genes[g].nsites, use_cg) : 0);
    const size_t budget = trim_hbm_budget(ctx);
    if (need > budget)
        return ctx->fail(PML_ENOMEM, "the pipeline keeps every gene resident through its stages: their bytes, flags and trimmed copies need " +
                                         std::to_string((need + ((size_t)1 << 20) - 1) >> 20) + " MiB of HBM, the budget is " + std::to_string(budget >> 20) + " MiB");
    auto emptied = [&](int g, const char *stage) {
        return ctx->fail(PML_EPARSE, "gene " + std::to_string(g) + " has no columns left after the " + stage + " stage, and another stage follows");
    };
    GbBatch gb; gb.ctx = ctx;
    TrimBatch tb; tb.ctx = ctx;
    std::vector<CgGene> last((size_t)ngenes);      // what the congruence stage reads
    if (use_gb) {
        if ((rc = gb.run(genes, 0, ngenes, gbp, use_cg ? &plan : nullptr, gb_result != nullptr))) return rc;
        for (int g = 0; g < ngenes; ++g) {
            if (gb.nkept[g] == 0 && (use_trim || use_cg)) return emptied(g, "Gblocks");
            last[(size_t)g] = CgGene{(const uint8_t *)(gb.d + gb.o_out[g]), use_cg ? (const uint16_t *)(gb.d + gb.o_map[g]) : nullptr, gb.nmap[g], gb.nkept[g], (int)gb.ld_out[g], 0};
        }
    }
    if (use_trim) {
        if (use_gb) {                              // on the matrices the Gblocks stage left in HBM
            std::vector<TrimResident> in((size_t)ngenes);
            for (int g = 0; g < ngenes; ++g) in[(size_t)g] = TrimResident{last[(size_t)g].bytes, last[(size_t)g].map, gb.nmap[g], gb.nkept[g], gb.ld_out[g]};
            rc = tb.classify(genes, 0, ngenes, use_cg ? &plan : nullptr, &in, &gb.rowsrc);
        } else rc = tb.classify(genes, 0, ngenes, use_cg ? &plan : nullptr);
        if (rc) return rc;
        if ((rc = tb.gather(mode, trim_result != nullptr))) return rc;
        for (int g = 0; g < ngenes; ++g) {
            if (tb.nkept[g] == 0 && use_cg) return emptied(g, "column filter");
            last[(size_t)g] = CgGene{(const uint8_t *)(tb.d + tb.o_out[g]), tb.map_ptr[(size_t)g], tb.nmap[g], tb.nkept[g], (int)tb.ld_out[g], 0};
        }
    }
    if (use_cg) {
        if ((rc = cg_costs_resident(pctx, plan, last, gb.bytes + tb.bytes, res))) return rc;
        rc = pml_congruence_select(ngenes, res->mean_cost, trim_percent, keep_out, nullptr, nullptr);
        if (rc) return ctx->fail(rc, "trim_percent puts the percentile index outside the genes (the reference throws)");
    }
    if (use_gb && gb_result && (trim_result_alloc(gb_result, ngenes) || gb.fill(gb_result))) return ctx->fail(PML_ENOMEM, "host allocation failed");
    if (use_trim && trim_result && (trim_result_alloc(trim_result, ngenes) || tb.fill(trim_result))) return ctx->fail(PML_ENOMEM, "host allocation failed");
    return PML_OK;
}
}  // namespace

extern "C" int pml_trim_pipeline(pml_ctx *pctx, int ngenes, const pml_alignment *genes, const pml_gblocks_params *gb, int use_gblocks, int mode, double trim_percent,
                                 int *keep_out, pml_trim_result *gb_result, pml_trim_result *trim_result, pml_congruence_result *congruence_result) {
    if (gb_result) std::memset(gb_result, 0, sizeof *gb_result);
    if (trim_result) std::memset(trim_result, 0, sizeof *trim_result);
    if (congruence_result) std::memset(congruence_result, 0, sizeof *congruence_result);
    if (!pctx || !genes || ngenes < 1) return PML_EINVAL;
    std::lock_guard<std::mutex> lk(pctx->c.mu);
    Ctx *ctx = &pctx->c;
    if (mode < -1 || mode > PML_TRIM_TOPOLOGICAL) return ctx->fail(PML_EINVAL, "mode must be -1 (no column filter), PML_TRIM_UNIFORM, PML_TRIM_GAP_UNIFORM or PML_TRIM_TOPOLOGICAL");
    if (!(trim_percent >= 0)) return ctx->fail(PML_EINVAL, "trim_percent must be positive, or 0 for no congruence stage");
    if (!use_gblocks && mode < 0 && !(trim_percent > 0)) return ctx->fail(PML_EINVAL, "no stage asked for");
    if (trim_percent > 0 && !keep_out) return ctx->fail(PML_EINVAL, "the congruence stage needs keep_out");
    pml_fpguard fpg;
    pml_drop_worker_caches(pctx);
    pml_congruence_result local;
    pml_congruence_result *res = congruence_result ? congruence_result : &local;
    std::memset(res, 0, sizeof *res);
    int rc;
    try { rc = pipeline_locked(pctx, ngenes, genes, gb, use_gblocks != 0, mode, trim_percent, keep_out, gb_result, trim_result, res); }
    catch (const std::bad_alloc &) { rc = ctx->fail(PML_ENOMEM, "host allocation failed"); }
    catch (const std::exception &e) { rc = ctx->fail(PML_EINVAL, e.what()); }
    if (rc || !congruence_result) pml_congruence_result_free(res);
    if (rc) { if (gb_result) pml_trim_result_free(gb_result); if (trim_result) pml_trim_result_free(trim_result); }
    return rc;
}

extern "C" int pml_debug_column_flags(pml_ctx *pctx, const pml_alignment *gene, unsigned char *flags_out) {
    if (!pctx || !gene || !flags_out) return PML_EINVAL;
    std::lock_guard<std::mutex> lk(pctx->c.mu);
    Ctx *ctx = &pctx->c;
    pml_fpguard fpg;
    pml_drop_worker_caches(pctx);
    try {
        if (int rc = trim_check_gene(ctx, *gene, 0)) return rc;
        TrimBatch tb; tb.ctx = ctx;
        if (int rc = tb.classify(gene, 0, 1, nullptr)) return rc;
        std::copy(tb.flags.begin(), tb.flags.end(), flags_out);
    } catch (const std::bad_alloc &) { return ctx->fail(PML_ENOMEM, "host allocation failed"); }
    catch (const std::exception &e) { return ctx->fail(PML_EINVAL, e.what()); }
    return PML_OK;
}

extern "C" int pml_trim_column_flags_host(const pml_alignment *gene, unsigned char *flags_out) {
    if (!gene || !flags_out || !gene->rows || gene->ntax <= 0 || gene->nsites < 0) return PML_EINVAL;
    for (int i = 0; i < gene->ntax; ++i) if (!gene->rows[i] || (int)strnlen(gene->rows[i], (size_t)gene->nsites) < gene->nsites) return PML_EINVAL;
    host_flags(*gene, flags_out);
    return PML_OK;
}

extern "C" int pml_trim_stats(pml_ctx *ctx, long long *class_launches, long long *gather_launches, double *total_ms) {
    if (!ctx) return PML_EINVAL;
    std::lock_guard<std::mutex> lk(ctx->c.mu);
    if (class_launches) *class_launches = ctx->c.colclass_launches;
    if (gather_launches) *gather_launches = ctx->c.colgather_launches;
    if (total_ms) for (int k = 0; k < 3; ++k) total_ms[k] = ctx->c.trim_ms[k];
    return PML_OK;
}
