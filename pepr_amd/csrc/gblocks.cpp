// gblocks.cpp -- the host half of block trimming (include/peprml.h): pml_gblocks_defaults, pml_gblocks_trim, pml_debug_gblocks_flags,
// pml_gblocks_flags_host, pml_gblocks_chunk, pml_gblocks_stats.  The kernels are gblocks.hip, the rules gblocks.hpp.
// A sub-batch of genes is resident as ONE allocation whose layout is known before anything runs: the genes in the CgGene layout,
// one class / stage byte per column, every gene's source columns (ld ints), its scratch slice where it has more than GB_LDS_COLS
// columns, and its trimmed matrix at the input's size.  k_gbselect writes nkept and ld_out into the TgGene records that
// k_colgather reads and the gather's tile list covers the input's width, so upload, three launches and the downloads are
// enqueued without a host step in between; tiles beyond a gene's ld_out return at once.
#include <algorithm>
#include <climits>
#include <cstring>

#include "../../include/peprml.h"
#include "api_types.hpp"
#include "trim.hpp"
#include "trim_dev.hpp"

using namespace pml;

namespace pml {

#define GBCHK(expr)                                                                                                   \
    do { hipError_t e_ = (expr);                                                                                      \
         if (e_ != hipSuccess) return ctx->fail(PML_EDEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); } while (0)

static GbParams params_in(const pml_gblocks_params *p) {
    return p ? GbParams{p->b1, p->b2, p->b3, p->b4, p->b0, p->gaps} : GbParams{0, 0, 0, 0, 0, 0};
}

static int resolve(Ctx *ctx, int n, const pml_gblocks_params *p, int g, GbParams &out) {
    const GbParams in = params_in(p);
    if (gb_resolve(n, &in, out) == 0) return PML_OK;
    const std::string msg = "gene " + std::to_string(g) + " (" + std::to_string(n) + " rows): b1 = " + std::to_string(out.b1) + ", b2 = " + std::to_string(out.b2) +
                            ", b3 = " + std::to_string(out.b3) + ", b4 = " + std::to_string(out.b4) + ", b0 = " + std::to_string(out.b0) + ", gaps = " +
                            std::to_string(out.gaps) + " are outside n / 2 < b1 <= b2 <= n, b3 >= 0, b4 >= 2, b0 >= 2, gaps in 1..3";
    return ctx ? ctx->fail(PML_EINVAL, msg) : PML_EINVAL;
}

size_t gb_gene_cost(int ntax, int ncols, bool with_map) {
    const size_t ld = align_up((size_t)ncols, 16);
    size_t b = 2 * align_up((size_t)ntax * ld, 256) + align_up(ld * sizeof(int), 256) + (size_t)ncols;
    if (ncols > GB_LDS_COLS) b += align_up(2 * (size_t)ncols * sizeof(int), 256);
    if (with_map) b += align_up((size_t)ntax * sizeof(uint16_t), 256);
    b += sizeof(int) * (size_t)((ncols + TRIM_COLS - 1) / TRIM_COLS) + sizeof(TgTile) * (size_t)trim_gather_tiles(ntax, ld);
    return b + sizeof(CgGene) + sizeof(GbGene) + sizeof(TgGene) + sizeof(long long) + sizeof(int);
}

GbBatch::~GbBatch() { if (d) hipFree(d); }

int GbBatch::run(const pml_alignment *genes, int first_, int count, const pml_gblocks_params *params, const CgPlan *plan, bool download) {
    first = first_; ng = count;
    ntax.resize(ng); nmap.assign(ng, 0); ncols.resize(ng); rowsrc.assign(ng, {}); ld.resize(ng); o_bytes.resize(ng); o_map.assign(ng, 0);
    o_out.assign(ng, 0); nkept.assign(ng, 0); ld_out.assign(ng, 0); kept.assign(ng, {});
    std::vector<GbParams> gp((size_t)ng);
    long long tiles = 0, total_cols = 0, gtiles = 0;
    for (int i = 0; i < ng; ++i) {
        const pml_alignment &A = genes[first + i];
        if (int rc = resolve(ctx, A.ntax, params, first + i, gp[(size_t)i])) return rc;
        ntax[i] = A.ntax; ncols[i] = A.nsites; ld[i] = align_up((size_t)A.nsites, 16);
        total_cols += A.nsites; tiles += (A.nsites + TRIM_COLS - 1) / TRIM_COLS; gtiles += A.nsites ? trim_gather_tiles(A.ntax, ld[i]) : 0;
        std::vector<int> &rs = rowsrc[i];
        if (plan) {                                // the rows the congruence stage reads first, a repeated name's earlier rows behind them
            std::vector<char> taken((size_t)A.ntax, 0);
            for (auto &ur : plan->order[(size_t)(first + i)]) { rs.push_back(ur.second); taken[(size_t)ur.second] = 1; }
            nmap[i] = (int)rs.size();
            for (int r = 0; r < A.ntax; ++r) if (!taken[(size_t)r]) rs.push_back(r);
        } else for (int r = 0; r < A.ntax; ++r) rs.push_back(r);
    }
    if (tiles > INT_MAX || gtiles > INT_MAX) return ctx->fail(PML_EINVAL, "too many columns for one call");
    const int ntiles = (int)tiles, ngt = (int)gtiles;
    // the uploaded part: descriptors, tile lists, maps and bytes
    size_t off = align_up((size_t)ng * sizeof(CgGene), 256);
    const size_t o_gb = off; off += align_up((size_t)ng * sizeof(GbGene), 256);
    const size_t o_tg = off; off += align_up((size_t)ng * sizeof(TgGene), 256);
    const size_t o_tt = off; off += align_up((size_t)ngt * sizeof(TgTile), 256);
    const size_t o_tiles = off; off += align_up((size_t)ntiles * sizeof(int), 256);
    const size_t o_first = off; off += align_up((size_t)ng * sizeof(int), 256);
    for (int i = 0; i < ng; ++i) {
        if (plan) { o_map[i] = off; off += align_up((size_t)nmap[i] * sizeof(uint16_t), 256); }
        o_bytes[i] = off; off += align_up((size_t)ntax[i] * ld[i], 256);
    }
    const size_t in_bytes = off;
    // what the kernels write
    const size_t o_flags = off; off += align_up((size_t)total_cols, 256);
    const size_t o_gom = off; off += align_up((size_t)ng * sizeof(long long), 256);
    const size_t o_src0 = off;
    std::vector<size_t> o_src((size_t)ng), o_scr((size_t)ng, 0);
    for (int i = 0; i < ng; ++i) { o_src[(size_t)i] = off; off += align_up(ld[i] * sizeof(int), 256); }
    const size_t o_src1 = off;
    for (int i = 0; i < ng; ++i) if (ncols[i] > GB_LDS_COLS) { o_scr[(size_t)i] = off; off += align_up(2 * (size_t)ncols[i] * sizeof(int), 256); }
    out0 = off;
    for (int i = 0; i < ng; ++i) { o_out[i] = off; off += align_up((size_t)ntax[i] * ld[i], 256); }
    bytes = off;
    GBCHK(hipSetDevice(ctx->device));
    GBCHK(hipMalloc((void **)&d, bytes));
    std::vector<char> host(in_bytes, 0);
    int *tile_gene = (int *)(host.data() + o_tiles), *tile_first = (int *)(host.data() + o_first);
    TgTile *tt = (TgTile *)(host.data() + o_tt);
    long long col_base = 0; int t = 0, nt = 0;
    for (int i = 0; i < ng; ++i) {
        const pml_alignment &A = genes[first + i];
        for (int p = 0; p < ntax[i]; ++p) std::memcpy(host.data() + o_bytes[i] + (size_t)p * ld[i], A.rows[rowsrc[i][(size_t)p]], (size_t)ncols[i]);
        if (plan) {
            uint16_t *map = (uint16_t *)(host.data() + o_map[i]);
            for (int p = 0; p < nmap[i]; ++p) map[p] = (uint16_t)plan->order[(size_t)(first + i)][(size_t)p].first;
        }
        ((CgGene *)host.data())[i] = CgGene{(const uint8_t *)(d + o_bytes[i]), plan ? (const uint16_t *)(d + o_map[i]) : nullptr, ntax[i], ncols[i], (int)ld[i], col_base};
        ((GbGene *)(host.data() + o_gb))[i] = GbGene{ntax[i], ncols[i], col_base, (int *)(d + o_src[(size_t)i]),
                                                     ncols[i] > GB_LDS_COLS ? (int *)(d + o_scr[(size_t)i]) : nullptr, gp[(size_t)i]};
        // nkept and ld_out are k_gbselect's to write
        ((TgGene *)(host.data() + o_tg))[i] = TgGene{(const uint8_t *)(d + o_bytes[i]), (uint8_t *)(d + o_out[i]), (const int *)(d + o_src[(size_t)i]), ntax[i], 0, (int)ld[i], 0};
        tile_first[i] = t;
        for (int k = 0; k < (ncols[i] + TRIM_COLS - 1) / TRIM_COLS; ++k) tile_gene[t++] = i;
        if (ncols[i])                              // the gather's tiles over the input's width: ld_out <= ld
            for (int q = 0; q < (int)(ld[i] / 16); q += TRIM_CHUNKS)
                for (int r = 0; r < ntax[i]; r += TRIM_ROWS) tt[nt++] = TgTile{i, q, r, 0};
        col_base += ncols[i];
    }
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    if (ctx->profile) for (auto &e : ev) e = ctx->get_event();
    struct Back { Ctx *c; hipEvent_t *e; ~Back() { for (int k = 0; k < 5; ++k) if (e[k]) c->pool.push_back(e[k]); } } back{ctx, ev};
    if (ev[0]) hipEventRecord(ev[0], ctx->stream);
    GBCHK(hipMemcpyAsync(d, host.data(), in_bytes, hipMemcpyHostToDevice, ctx->stream));
    if (ev[1]) hipEventRecord(ev[1], ctx->stream);
    GBCHK(hipMemsetAsync(d + o_gom, 0, (size_t)ng * sizeof(long long), ctx->stream));
    launch_gbclass((const CgGene *)d, (const GbGene *)(d + o_gb), (const int *)(d + o_tiles), (const int *)(d + o_first), ntiles, (uint8_t *)(d + o_flags),
                   (long long *)(d + o_gom), ctx->stream);
    if (ev[2]) hipEventRecord(ev[2], ctx->stream);
    launch_gbselect((const GbGene *)(d + o_gb), ng, (uint8_t *)(d + o_flags), (TgGene *)(d + o_tg), ctx->stream);
    if (ev[3]) hipEventRecord(ev[3], ctx->stream);
    launch_colgather((const TgGene *)(d + o_tg), (const TgTile *)(d + o_tt), nt, ctx->stream);
    if (ev[4]) hipEventRecord(ev[4], ctx->stream);
    if (ntiles > 0) ctx->gbclass_launches++;
    ctx->gbselect_launches++;
    if (nt > 0) ctx->colgather_launches++;
    GBCHK(hipGetLastError());
    flags.resize((size_t)total_cols); gom.resize((size_t)ng);
    std::vector<TgGene> tg((size_t)ng);
    std::vector<char> src_host(o_src1 - o_src0);
    if (total_cols) GBCHK(hipMemcpyAsync(flags.data(), d + o_flags, flags.size(), hipMemcpyDeviceToHost, ctx->stream));
    GBCHK(hipMemcpyAsync(gom.data(), d + o_gom, gom.size() * sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
    GBCHK(hipMemcpyAsync(tg.data(), d + o_tg, tg.size() * sizeof(TgGene), hipMemcpyDeviceToHost, ctx->stream));
    if (total_cols) GBCHK(hipMemcpyAsync(src_host.data(), d + o_src0, src_host.size(), hipMemcpyDeviceToHost, ctx->stream));
    if (ctx->sync(ctx->stream)) return PML_EDEVICE;
    if (ev[0]) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) ctx->gb_ms[2] += ms;
        if (hipEventElapsedTime(&ms, ev[1], ev[2]) == hipSuccess) ctx->gb_ms[0] += ms;
        if (hipEventElapsedTime(&ms, ev[2], ev[3]) == hipSuccess) ctx->gb_ms[1] += ms;
        if (nt > 0 && hipEventElapsedTime(&ms, ev[3], ev[4]) == hipSuccess) ctx->trim_ms[1] += ms;
    }
    size_t out1 = out0;
    for (int i = 0; i < ng; ++i) {
        nkept[i] = tg[(size_t)i].nkept; ld_out[i] = (size_t)tg[(size_t)i].ld_out;
        if (nkept[i] < 0 || nkept[i] > ncols[i] || ld_out[i] != align_up((size_t)nkept[i], 16))
            return ctx->fail(PML_EDEVICE, "internal: k_gbselect left an impossible column count for gene " + std::to_string(first + i));
        const int *src = (const int *)(src_host.data() + (o_src[(size_t)i] - o_src0));
        kept[i].assign(src, src + nkept[i]);
        if (nkept[i]) out1 = o_out[i] + (size_t)ntax[i] * ld_out[i];
    }
    if (download && out1 > out0) {
        out_host.resize(out1 - out0);
        GBCHK(hipMemcpyAsync(out_host.data(), d + out0, out_host.size(), hipMemcpyDeviceToHost, ctx->stream));
        if (ctx->sync(ctx->stream)) return PML_EDEVICE;
    }
    return PML_OK;
}

int GbBatch::fill(pml_trim_result *res) const {
    for (int i = 0; i < ng; ++i)
        if (trim_fill_gene(res, first + i, ntax[i], ncols[i], gom[i], kept[i], rowsrc[i], nkept[i] ? out_host.data() + (o_out[i] - out0) : nullptr, ld_out[i]))
            return PML_ENOMEM;
    return PML_OK;
}

}  // namespace pml

namespace {

int gb_trim_locked(pml_ctx *pctx, int ngenes, const pml_alignment *genes, const pml_gblocks_params *params, pml_trim_result *result) {
    Ctx *ctx = &pctx->c;
    for (int g = 0; g < ngenes; ++g) {
        if (int rc = trim_check_gene(ctx, genes[g], g)) return rc;
        GbParams p;
        if (int rc = resolve(ctx, genes[g].ntax, params, g, p)) return rc;
    }
    const size_t budget = trim_hbm_budget(ctx);
    if (trim_result_alloc(result, ngenes)) return ctx->fail(PML_ENOMEM, "host allocation failed");
    for (int g0 = 0; g0 < ngenes;) {
        size_t need = TRIM_BATCH_SLACK; int g1 = g0;
        while (g1 < ngenes) {
            const size_t c = gb_gene_cost(genes[g1].ntax, genes[g1].nsites, false);
            if (need + c > budget) break;
            need += c; ++g1;
        }
        if (g1 == g0) {
            const size_t c = TRIM_BATCH_SLACK + gb_gene_cost(genes[g0].ntax, genes[g0].nsites, false);
            return ctx->fail(PML_ENOMEM, "gene " + std::to_string(g0) + " (" + std::to_string(genes[g0].ntax) + " rows, " + std::to_string(genes[g0].nsites) +
                                             " columns) needs " + std::to_string((c + ((size_t)1 << 20) - 1) >> 20) + " MiB of HBM for its bytes, flags and trimmed copy, the budget is " +
                                             std::to_string(budget >> 20) + " MiB");
        }
        GbBatch gb; gb.ctx = ctx;
        if (int rc = gb.run(genes, g0, g1 - g0, params, nullptr, true)) return rc;
        if (gb.fill(result)) return ctx->fail(PML_ENOMEM, "host allocation failed");
        g0 = g1;
    }
    return PML_OK;
}

}  // namespace

extern "C" int pml_gblocks_defaults(int ntax, pml_gblocks_params *out) {
    if (!out) return PML_EINVAL;
    GbParams p;
    if (gb_resolve(ntax, nullptr, p)) return PML_EINVAL;
    *out = pml_gblocks_params{p.b1, p.b2, p.b3, p.b4, p.b0, p.gaps};
    return PML_OK;
}

extern "C" int pml_gblocks_chunk(void) { return GB_CHUNK; }

extern "C" int pml_gblocks_trim(pml_ctx *ctx, int ngenes, const pml_alignment *genes, const pml_gblocks_params *params, pml_trim_result *result) {
    if (result) std::memset(result, 0, sizeof *result);
    if (!ctx || !genes || ngenes < 1 || !result) return PML_EINVAL;
    std::lock_guard<std::mutex> lk(ctx->c.mu);
    pml_fpguard fpg;
    pml_drop_worker_caches(ctx);
    int rc;
    try { rc = gb_trim_locked(ctx, ngenes, genes, params, result); }
    catch (const std::bad_alloc &) { rc = ctx->c.fail(PML_ENOMEM, "host allocation failed"); }
    catch (const std::exception &e) { rc = ctx->c.fail(PML_EINVAL, e.what()); }
    if (rc) pml_trim_result_free(result);
    return rc;
}

extern "C" int pml_debug_gblocks_flags(pml_ctx *pctx, const pml_alignment *gene, const pml_gblocks_params *params, unsigned char *flags_out) {
    if (!pctx || !gene || !flags_out) return PML_EINVAL;
    std::lock_guard<std::mutex> lk(pctx->c.mu);
    Ctx *ctx = &pctx->c;
    pml_fpguard fpg;
    pml_drop_worker_caches(pctx);
    try {
        if (int rc = trim_check_gene(ctx, *gene, 0)) return rc;
        GbBatch gb; gb.ctx = ctx;
        if (int rc = gb.run(gene, 0, 1, params, nullptr, false)) return rc;
        std::copy(gb.flags.begin(), gb.flags.end(), flags_out);
    } catch (const std::bad_alloc &) { return ctx->fail(PML_ENOMEM, "host allocation failed"); }
    catch (const std::exception &e) { return ctx->fail(PML_EINVAL, e.what()); }
    return PML_OK;
}

extern "C" int pml_gblocks_flags_host(const pml_alignment *gene, const pml_gblocks_params *params, unsigned char *flags_out) {
    if (!gene || !flags_out || !gene->rows || gene->ntax <= 0 || gene->nsites < 0) return PML_EINVAL;
    for (int i = 0; i < gene->ntax; ++i) if (!gene->rows[i] || (int)strnlen(gene->rows[i], (size_t)gene->nsites) < gene->nsites) return PML_EINVAL;
    GbParams p;
    if (resolve(nullptr, gene->ntax, params, 0, p)) return PML_EINVAL;
    const int L = gene->nsites, n = gene->ntax;
    try {
        std::vector<unsigned> f((size_t)L);
        for (int c = 0; c < L; ++c) {                  // the exact counts, from a histogram
            int count[256] = {0}, top = 0;
            for (int r = 0; r < n; ++r) count[(unsigned char)gene->rows[r][c]]++;
            for (int b = 0; b < 256; ++b) if (b != '-') top = std::max(top, count[b]);
            f[(size_t)c] = gb_class(count['-'], top, n, p);
        }
        std::vector<int> prev_a((size_t)L), prev_b((size_t)L);
        for (int r = 1; r <= GB_ROUNDS; ++r) {         // the same rounds with sequential scans
            int a = -1, b = -1;
            for (int c = 0; c < L; ++c) {
                bool A, B;
                gb_round_in(r, f[(size_t)c], A, B);
                if (A) a = c;
                if (B) b = c;
                prev_a[(size_t)c] = a; prev_b[(size_t)c] = b;
            }
            a = b = L;
            for (int c = L - 1; c >= 0; --c) {
                bool A, B;
                gb_round_in(r, f[(size_t)c], A, B);
                if (A) a = c;
                if (B) b = c;
                f[(size_t)c] = gb_round_out(r, f[(size_t)c], prev_a[(size_t)c], prev_b[(size_t)c], a, b, p);
            }
        }
        for (int c = 0; c < L; ++c) flags_out[c] = (unsigned char)f[(size_t)c];
    } catch (const std::bad_alloc &) { return PML_ENOMEM; }
    return PML_OK;
}

extern "C" int pml_gblocks_stats(pml_ctx *ctx, long long *class_launches, long long *select_launches, double *total_ms) {
    if (!ctx) return PML_EINVAL;
    std::lock_guard<std::mutex> lk(ctx->c.mu);
    if (class_launches) *class_launches = ctx->c.gbclass_launches;
    if (select_launches) *select_launches = ctx->c.gbselect_launches;
    if (total_ms) for (int k = 0; k < 3; ++k) total_ms[k] = ctx->c.gb_ms[k];
    return PML_OK;
}
