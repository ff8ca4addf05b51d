// sw.cpp -- the device driver of the homology search (include/peprml.h "Homology search"): pml_sw_search, pml_debug_sw_scores,
// pml_sw_stats.  The kernel is sw.hip; encoding, statistics, table text and traceback sw_host.cpp.  Resident for the call: the
// queries' codes, every genome's subject stream (subjects ordered by length, SW_MARK behind each, cut into chunks of a bounded
// byte count), the per-subject positions, the chunk and query records and the nq x G keys -- the only download.  Work is cut into
// units (a range of a class's queries x a range of chunks) of a bounded cell count whose line buffers fit the HBM budget; a unit
// is one launch.  PML_SW_TINY_UNITS=1 (test hook) makes chunks of 40 stream bytes and units of 3 queries x 2 chunks.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "../../include/peprml.h"
#include "api_types.hpp"
#include "trim_dev.hpp"

using namespace pml;

namespace {

#define SCHK(expr)                                                                                                    \
    do { hipError_t e_ = (expr);                                                                                      \
         if (e_ != hipSuccess) return ctx->fail(PML_EDEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); } while (0)

struct DevBuf {
    char *d = nullptr;
    ~DevBuf() { if (d) hipFree(d); }
};

struct Subject { const uint8_t *codes; int len, pos; };
struct Queries { const uint8_t *codes; size_t code_bytes; std::vector<long long> off; std::vector<int> len; };

int class_of(int len) { return len <= SW_LANES[0] * SW_STRIP ? 0 : len <= SW_LANES[1] * SW_STRIP ? 1 : 2; }

// best[q * G + g] of every query against every genome's subjects; dbg (test door): [nq][dbg_ld] raw scores by position
int score_all(Ctx *ctx, const Queries &Q, const std::vector<std::vector<Subject>> &genomes, const SwOpts &o, int force_class, std::vector<unsigned long long> &best,
              std::vector<int> *dbg, int dbg_ld) {
    const int nq = (int)Q.len.size(), G = (int)genomes.size();
    best.assign((size_t)nq * std::max(G, 1), 0ull);
    if (dbg) dbg->assign((size_t)nq * std::max(dbg_ld, 1), 0);
    const bool tiny = std::getenv("PML_SW_TINY_UNITS") && std::atoi(std::getenv("PML_SW_TINY_UNITS")) != 0;
    const int chunk_bytes = tiny ? 40 : SW_CHUNK_DEFAULT;
    const long long unit_cells = SW_UNIT_CELLS_DEFAULT;
    const int range_chunks = tiny ? 2 : 32768, unit_queries = tiny ? 3 : (1 << 22);
    const long long range_len = 1LL << 20;
    // the streams and their chunks
    std::vector<uint8_t> stream; std::vector<int> sub_pos; std::vector<SwChunk> chunks;
    for (int g = 0; g < G; ++g) {
        std::vector<Subject> subs;
        for (const Subject &s : genomes[(size_t)g]) if (s.len > 0) subs.push_back(s);
        std::stable_sort(subs.begin(), subs.end(), [](const Subject &a, const Subject &b) { return a.len < b.len; });
        SwChunk cur; cur.len = 0;
        for (const Subject &s : subs) {
            if (cur.len > 0 && cur.len + s.len + 1 > chunk_bytes) { chunks.push_back(cur); cur.len = 0; }
            if (cur.len == 0) { cur.off = (long long)stream.size(); cur.sub0 = (int)sub_pos.size(); cur.genome = g; cur.lb_at = 0; }
            stream.insert(stream.end(), s.codes, s.codes + s.len);
            stream.push_back((uint8_t)SW_MARK);
            sub_pos.push_back(s.pos);
            cur.len += s.len + 1;
        }
        if (cur.len > 0) chunks.push_back(cur);
    }
    if (stream.size() > ((size_t)1 << 30)) return ctx->fail(PML_EINVAL, "more than 2^30 subject residues in one call");
    // chunk ranges: a grid dimension, and the line buffer of one query of several passes
    std::vector<int> range_at(1, 0);
    long long max_range = 0, acc = 0;
    for (size_t c = 0; c < chunks.size(); ++c) {
        if ((int)c > range_at.back() && ((int)c - range_at.back() >= range_chunks || acc + chunks[c].len > range_len)) { range_at.push_back((int)c); acc = 0; }
        chunks[c].lb_at = (int)acc;
        acc += chunks[c].len;
        max_range = std::max(max_range, acc);
    }
    range_at.push_back((int)chunks.size());
    // the classes' query lists, by length
    std::vector<int> order[SW_CLASSES];
    for (int q = 0; q < nq; ++q) {
        if (Q.len[(size_t)q] <= 0) continue;
        const int cls = force_class >= 0 ? force_class : class_of(Q.len[(size_t)q]);
        if (cls < SW_CLASSES - 1 && Q.len[(size_t)q] > SW_LANES[cls] * SW_STRIP)
            return ctx->fail(PML_EINVAL, "a query of " + std::to_string(Q.len[(size_t)q]) + " residues does not fit class " + std::to_string(cls) + " (" +
                                             std::to_string(SW_LANES[cls] * SW_STRIP) + " rows in its one pass)");
        order[cls].push_back(q);
    }
    if (chunks.empty() || (order[0].empty() && order[1].empty() && order[2].empty())) return PML_OK;
    SCHK(hipSetDevice(ctx->device));
    const size_t budget = trim_hbm_budget(ctx);
    size_t off = 0;
    const size_t nqa = order[0].size() + order[1].size() + order[2].size();
    const size_t o_best = off; off += align_up(best.size() * sizeof(unsigned long long), 256);
    const size_t o_queries = off; off += align_up(nqa * sizeof(SwQuery), 256);
    const size_t o_chunks = off; off += align_up(chunks.size() * sizeof(SwChunk), 256);
    const size_t o_subpos = off; off += align_up(sub_pos.size() * sizeof(int), 256);
    const size_t o_dbg = off; off += dbg ? align_up(dbg->size() * sizeof(int), 256) : 0;
    const size_t o_table = off; off += align_up((size_t)SW_TROWS * SW_TSTRIDE, 256);
    const size_t o_codes = off; off += align_up(std::max<size_t>(Q.code_bytes, 1), 256);
    const size_t o_stream = off; off += align_up(stream.size(), 256);
    const size_t o_lb = off;
    if (off + 2 * (size_t)max_range * sizeof(int2) > budget)
        return ctx->fail(PML_ENOMEM, "the call's " + std::to_string(stream.size()) + " subject residues and " + std::to_string(best.size()) + " keys need " +
                                         std::to_string((off >> 20) + 1) + " MiB of HBM, the budget is " + std::to_string(budget >> 20) + " MiB");
    const size_t lb_budget = std::min<size_t>((budget - off) / 2, (size_t)1 << 30);
    // units: per class, ranges of its list
    struct Unit { int cls; size_t q0, q1; };
    std::vector<Unit> units; std::vector<SwQuery> hq;
    size_t lb_need = 0;
    for (int cls = 0; cls < SW_CLASSES; ++cls) {
        std::stable_sort(order[cls].begin(), order[cls].end(), [&](int a, int b) { return Q.len[(size_t)a] < Q.len[(size_t)b]; });
        size_t q0 = hq.size(); long long rows = 0, nlb = 0;
        for (int q : order[cls]) {
            const int len = Q.len[(size_t)q];
            const bool multi = len > SW_LANES[cls] * SW_STRIP;
            if (hq.size() > q0 && ((rows + len) * max_range > unit_cells || (multi && (size_t)(nlb + 1) * max_range * sizeof(int2) > lb_budget) ||
                                   (int)(hq.size() - q0) >= unit_queries)) {
                units.push_back({cls, q0, hq.size()}); q0 = hq.size(); rows = 0; nlb = 0;
            }
            SwQuery r; r.off = Q.off[(size_t)q]; r.len = len; r.index = q; r.lb_off = multi ? nlb++ * max_range : -1;
            hq.push_back(r); rows += len;
            lb_need = std::max(lb_need, (size_t)nlb * (size_t)max_range * sizeof(int2));
        }
        if (hq.size() > q0) units.push_back({cls, q0, hq.size()});
    }
    int8_t tab8[SW_TROWS * SW_TSTRIDE] = {0};
    for (int i = 0; i < 24; ++i) for (int j = 0; j < 24; ++j) tab8[i * SW_TSTRIDE + j] = (int8_t)o.table[i * 24 + j];
    DevBuf buf;
    SCHK(hipMalloc((void **)&buf.d, std::max<size_t>(off + lb_need, 256)));
    char *d = buf.d;
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    if (ctx->profile) for (auto &e : ev) e = ctx->get_event();
    struct Back { Ctx *c; hipEvent_t *e; ~Back() { for (int i = 0; i < 5; ++i) if (e[i]) c->pool.push_back(e[i]); } } back{ctx, ev};
    if (ev[4]) hipEventRecord(ev[4], ctx->stream);
    SCHK(hipMemsetAsync(d + o_best, 0, o_queries - o_best, ctx->stream));
    SCHK(hipMemcpyAsync(d + o_queries, hq.data(), hq.size() * sizeof(SwQuery), hipMemcpyHostToDevice, ctx->stream));
    SCHK(hipMemcpyAsync(d + o_chunks, chunks.data(), chunks.size() * sizeof(SwChunk), hipMemcpyHostToDevice, ctx->stream));
    SCHK(hipMemcpyAsync(d + o_subpos, sub_pos.data(), sub_pos.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    if (dbg) SCHK(hipMemsetAsync(d + o_dbg, 0, o_table - o_dbg, ctx->stream));
    SCHK(hipMemcpyAsync(d + o_table, tab8, sizeof tab8, hipMemcpyHostToDevice, ctx->stream));
    if (Q.code_bytes) SCHK(hipMemcpyAsync(d + o_codes, Q.codes, Q.code_bytes, hipMemcpyHostToDevice, ctx->stream));
    SCHK(hipMemcpyAsync(d + o_stream, stream.data(), stream.size(), hipMemcpyHostToDevice, ctx->stream));
    if (ev[0]) hipEventRecord(ev[0], ctx->stream);
    size_t u = 0;
    for (int cls = 0; cls < SW_CLASSES; ++cls) {
        for (; u < units.size() && units[u].cls == cls; ++u)
            for (size_t r = 0; r + 1 < range_at.size(); ++r) {
                SwRun run; run.oe = o.open + o.ext; run.ext = o.ext; run.G = G; run.nq = (int)(units[u].q1 - units[u].q0); run.chunk0 = range_at[r]; run.pad = 0;
                run.lb_base = 0; run.dbg_ld = dbg_ld;
                launch_sw_score(cls, (const SwQuery *)(d + o_queries) + units[u].q0, (const SwChunk *)(d + o_chunks), range_at[r + 1] - range_at[r], run,
                                (const uint8_t *)(d + o_codes), (const uint8_t *)(d + o_stream), (const int *)(d + o_subpos), (const int8_t *)(d + o_table),
                                (int2 *)(d + o_lb), (unsigned long long *)(d + o_best), dbg ? (int *)(d + o_dbg) : nullptr, ctx->stream);
                ctx->sw_launches[cls]++; ctx->sw_launches[3]++;
            }
        if (ev[1 + cls]) hipEventRecord(ev[1 + cls], ctx->stream);
    }
    SCHK(hipGetLastError());
    SCHK(hipMemcpyAsync(best.data(), d + o_best, best.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    if (dbg) SCHK(hipMemcpyAsync(dbg->data(), d + o_dbg, dbg->size() * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    if (ctx->sync(ctx->stream)) return PML_EDEVICE;
    if (ev[0]) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, ev[4], ev[0]) == hipSuccess) ctx->sw_ms[3] += ms;
        for (int cls = 0; cls < SW_CLASSES; ++cls) if (hipEventElapsedTime(&ms, ev[cls], ev[1 + cls]) == hipSuccess) ctx->sw_ms[cls] += ms;
    }
    long long sres = 0, qres = 0;
    for (const SwChunk &c : chunks) sres += c.len;
    sres -= (long long)sub_pos.size();
    for (size_t c = 0; c < SW_CLASSES; ++c) for (int q : order[c]) qres += Q.len[(size_t)q];
    ctx->sw_cells += sres * qres;
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

}  // namespace

namespace pml {
int sw_scores_encoded(Ctx *ctx, const uint8_t *codes, const long long *off, const int *len, int n, const SwOpts &o, std::vector<int> &scores) {
    Queries Q; Q.codes = codes + off[0]; Q.code_bytes = (size_t)(off[n - 1] + len[n - 1] - off[0]);
    std::vector<std::vector<Subject>> genomes(1);
    for (int i = 0; i < n; ++i) { Q.off.push_back(off[i] - off[0]); Q.len.push_back(len[i]); genomes[0].push_back({codes + off[i], len[i], i}); }
    std::vector<unsigned long long> best;
    return score_all(ctx, Q, genomes, o, -1, best, &scores, n);
}
}  // namespace pml

extern "C" int pml_sw_search(pml_ctx *pctx, const pml_proteome_set *set, const pml_sw_opts *opts, pml_sw_result *result) {
    if (result) std::memset(result, 0, sizeof *result);
    if (!pctx || !set || !result) return PML_EINVAL;
    const int rc = guarded(pctx, [&](Ctx *ctx) -> int {
        SwOpts o; SwSet s; std::string err;
        if (!sw_resolve(opts, o, err) || !sw_encode(set, s, err)) return ctx->fail(PML_EINVAL, err);
        Queries Q; Q.codes = s.codes.data(); Q.code_bytes = s.codes.size();
        Q.off.assign(s.off.begin(), s.off.end() - 1);
        std::vector<std::vector<Subject>> genomes((size_t)s.G);
        for (int p = 0; p < s.np; ++p) {
            Q.len.push_back(s.len(p));
            genomes[(size_t)s.genome_of[(size_t)p]].push_back({s.codes.data() + s.off[(size_t)p], s.len(p), s.pos_in_genome[(size_t)p]});
        }
        std::vector<unsigned long long> best;
        if (int rc2 = score_all(ctx, Q, genomes, o, -1, best, nullptr, 0)) return rc2;
        const int rc3 = sw_finish(s, o, best, sw_total_cells(s), result, err);
        return rc3 ? ctx->fail(rc3, err) : PML_OK;
    });
    if (rc) pml_sw_result_free(result);
    return rc;
}

extern "C" int pml_debug_sw_scores(pml_ctx *pctx, int nq, const char *const *queries, int ns, const char *const *subjects, const pml_sw_opts *opts, int force_class,
                                   int force_path, int *scores_out) {
    if (!pctx || nq < 0 || ns < 0 || (nq > 0 && !queries) || (ns > 0 && !subjects) || (nq > 0 && ns > 0 && !scores_out)) return PML_EINVAL;
    return guarded(pctx, [&](Ctx *ctx) -> int {
        if (force_class < -1 || force_class >= SW_CLASSES) return ctx->fail(PML_EINVAL, "force_class is -1 .. 2");
        if (force_path != 0) return ctx->fail(PML_EINVAL, "force_path 0 (int32) is the only path built");
        SwOpts o; std::string err;
        if (!sw_resolve(opts, o, err)) return ctx->fail(PML_EINVAL, err);
        std::vector<uint8_t> qc, sc; std::vector<long long> soff(1, 0);
        Queries Q;
        auto encode = [&](const char *text, const char *what, int i, std::vector<uint8_t> &into) -> int {
            if (!text) return ctx->fail(PML_EINVAL, std::string("a null ") + what);
            const size_t n = std::strlen(text), at = into.size();
            if (n > (size_t)SW_MAX_LEN) return ctx->fail(PML_EINVAL, std::string(what) + " " + std::to_string(i) + " has " + std::to_string(n) + " residues, the limit is 65535");
            into.resize(at + n);
            long long bad = 0;
            if (sw_encode_residues(text, n, into.data() + at, &bad)) return ctx->fail(PML_EINVAL, std::string(what) + " " + std::to_string(i) + ": position " + std::to_string(bad) + " is no residue");
            return PML_OK;
        };
        for (int i = 0; i < nq; ++i) { Q.off.push_back((long long)qc.size()); if (int rc = encode(queries[i], "query", i, qc)) return rc; Q.len.push_back((int)(qc.size() - (size_t)Q.off.back())); }
        for (int i = 0; i < ns; ++i) { if (int rc = encode(subjects[i], "subject", i, sc)) return rc; soff.push_back((long long)sc.size()); }
        Q.codes = qc.data(); Q.code_bytes = qc.size();
        std::vector<std::vector<Subject>> genomes(1);
        for (int i = 0; i < ns; ++i) genomes[0].push_back({sc.data() + soff[(size_t)i], (int)(soff[(size_t)i + 1] - soff[(size_t)i]), i});
        std::vector<unsigned long long> best; std::vector<int> dbg;
        if (int rc = score_all(ctx, Q, genomes, o, force_class, best, &dbg, ns)) return rc;
        std::copy(dbg.begin(), dbg.begin() + (size_t)nq * ns, scores_out);
        return PML_OK;
    });
}

extern "C" int pml_sw_stats(pml_ctx *ctx, long long *launches, long long *cells, double *total_ms) {
    if (!ctx) return PML_EINVAL;
    std::lock_guard<std::mutex> lk(ctx->c.mu);
    if (launches) for (int i = 0; i < 4; ++i) launches[i] = ctx->c.sw_launches[i];
    if (cells) *cells = ctx->c.sw_cells;
    if (total_ms) for (int i = 0; i < 4; ++i) total_ms[i] = ctx->c.sw_ms[i];
    return PML_OK;
}
