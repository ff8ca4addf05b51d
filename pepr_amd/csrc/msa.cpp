// msa.cpp -- the device driver of the multiple alignment (include/peprml.h "Multiple alignment"): pml_msa_align,
// pml_msa_profile_align, pml_debug_msa_profile_align, pml_msa_stats.  The kernels are msa.hip; encoding, the guide tree, the bound
// and the result's layout msa_host.cpp.  A call's sets become jobs (starting clusters and merges); the pair scores of a set come
// from the homology search's launch path (sw_scores_encoded, consecutive sets grouped), the trees are built on the host, and every level of all trees is
// one round of launches: k_msa_colv, k_msa_dp, k_msa_walk per sub-batch of the direction-word scratch, then the merged lengths
// and scores come back (the only download between levels), the merged clusters are allocated at their exact size and one
// k_msa_gather writes them.  PML_MSA_SCRATCH_BYTES (test door) sets the scratch budget.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "../../include/peprml.h"
#include "api_types.hpp"
#include "msa.hpp"
#include "sw.hpp"
#include "trim_dev.hpp"

using namespace pml;

namespace {

#define MCHK(expr)                                                                                                    \
    do { hipError_t e_ = (expr);                                                                                      \
         if (e_ != hipSuccess) return ctx->fail(PML_EDEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); } while (0)

struct DevBufs {
    std::vector<void *> all;
    ~DevBufs() { for (void *p : all) if (p) hipFree(p); }
    void drop(void *p) { for (void *&q : all) if (q == p) { hipFree(q); q = nullptr; } }
};

inline size_t al(size_t n) { return (n + 255) & ~(size_t)255; }

struct Leaf { const uint8_t *rows; int n, L; };
struct Job {
    int set = 0;
    std::vector<Leaf> leaves;
    MsaPlan plan;
    MsaProfile fin;
    std::vector<uint8_t> path;
};
struct Node { uint8_t *rows; uint32_t *cnt; int n, L; };

int class_of(int LX) { return LX <= MSA_LANES[0] * MSA_STRIP ? 0 : LX <= MSA_LANES[1] * MSA_STRIP ? 1 : 2; }

int msa_run(Ctx *ctx, std::vector<Job> &jobs, const MsaOpts &o, int force_class, bool want_path) {
    MCHK(hipSetDevice(ctx->device));
    size_t scratch_budget = trim_hbm_budget(ctx) / 2;
    if (const char *e = std::getenv("PML_MSA_SCRATCH_BYTES")) scratch_budget = (size_t)std::atoll(e);
    DevBufs bufs;
    struct Ev { int kind; hipEvent_t a, b; };
    std::vector<Ev> evs;
    auto timed = [&](int kind, auto &&launch) {
        ctx->msa_counts[kind]++;
        if (!ctx->profile) { launch(); return; }
        Ev e{kind, ctx->get_event(), ctx->get_event()};
        hipEventRecord(e.a, ctx->stream); launch(); hipEventRecord(e.b, ctx->stream);
        evs.push_back(e);
    };
    auto resolve = [&]() {
        for (const Ev &e : evs) { float ms = 0; if (hipEventElapsedTime(&ms, e.a, e.b) == hipSuccess) ctx->msa_ms[e.kind] += ms; ctx->pool.push_back(e.a); ctx->pool.push_back(e.b); }
        evs.clear();
    };
    struct Resolve { decltype(resolve) &r; ~Resolve() { r(); } } at_exit{resolve};

    // the starting clusters: rows, counts
    size_t nleaves = 0, row_bytes = 0, cnt_bytes = 0; int max_L = 0, max_level = 0;
    for (const Job &j : jobs) {
        for (const Leaf &l : j.leaves) { ++nleaves; row_bytes += al((size_t)l.n * l.L); cnt_bytes += al((size_t)l.L * 48); max_L = std::max(max_L, l.L); }
        for (const MsaMerge &m : j.plan.merges) max_level = std::max(max_level, m.level);
    }
    const size_t o_rows = 0, o_cnt = o_rows + row_bytes, o_cl = o_cnt + cnt_bytes, o_tab = o_cl + al(nleaves * sizeof(MsaCluster)), base_bytes = o_tab + al(576);
    char *base = nullptr;
    MCHK(hipMalloc((void **)&base, base_bytes));
    bufs.all.push_back(base);
    std::vector<std::vector<Node>> nodes(jobs.size());
    {
        std::vector<uint8_t> stage(row_bytes, (uint8_t)MSA_GAP);
        std::vector<MsaCluster> cl; cl.reserve(nleaves);
        size_t ar = 0, ac = 0;
        for (size_t ji = 0; ji < jobs.size(); ++ji)
            for (const Leaf &l : jobs[ji].leaves) {
                std::memcpy(stage.data() + ar, l.rows, (size_t)l.n * l.L);
                Node nd{(uint8_t *)(base + o_rows + ar), (uint32_t *)(base + o_cnt + ac), l.n, l.L};
                nodes[ji].push_back(nd);
                cl.push_back(MsaCluster{nd.rows, nd.cnt, l.n, l.L});
                ar += al((size_t)l.n * l.L); ac += al((size_t)l.L * 48);
            }
        int8_t tab8[576];
        for (int i = 0; i < 576; ++i) tab8[i] = (int8_t)o.table[i];
        MCHK(hipMemcpyAsync(base + o_rows, stage.data(), row_bytes, hipMemcpyHostToDevice, ctx->stream));
        MCHK(hipMemcpyAsync(base + o_cl, cl.data(), cl.size() * sizeof(MsaCluster), hipMemcpyHostToDevice, ctx->stream));
        MCHK(hipMemcpyAsync(base + o_tab, tab8, sizeof tab8, hipMemcpyHostToDevice, ctx->stream));
        if (max_level > 0) timed(0, [&] { launch_msa_counts((const MsaCluster *)(base + o_cl), (int)nleaves, max_L, ctx->stream); });
        if (ctx->sync(ctx->stream)) return PML_EDEVICE;                  // the staging vectors leave scope
    }
    for (Job &j : jobs) j.plan.score.assign(j.plan.merges.size(), 0);

    char *dir = nullptr; size_t dir_bytes = 0;
    char *prev_level = nullptr;
    struct Ref { int job, merge; };
    for (int lv = 1; lv <= max_level; ++lv) {
        std::vector<Ref> refs;
        for (size_t ji = 0; ji < jobs.size(); ++ji)
            for (size_t m = 0; m < jobs[ji].plan.merges.size(); ++m) if (jobs[ji].plan.merges[m].level == lv) refs.push_back({(int)ji, (int)m});
        std::vector<MsaTask> tasks; std::vector<Ref> tref; std::vector<size_t> tdir;
        for (int cls = 0; cls < MSA_CLASSES; ++cls)
            for (const Ref &r : refs) {
                const Job &j = jobs[(size_t)r.job];
                const MsaMerge &m = j.plan.merges[(size_t)r.merge];
                const Node &X = nodes[(size_t)r.job][(size_t)m.x], &Y = nodes[(size_t)r.job][(size_t)m.y];
                const int c = force_class >= 0 ? force_class : class_of(X.L);
                if (c != cls) continue;
                const std::string who = "set " + std::to_string(j.set) + ", merge of clusters " + std::to_string(m.x) + " and " + std::to_string(m.y) + ": ";
                const std::string why = msa_refusal(X.n, Y.n, X.L, Y.L, o);
                if (!why.empty()) return ctx->fail(PML_EINVAL, who + why);
                const int lanes = MSA_LANES[c], pass_rows = lanes * MSA_STRIP;
                if (c < MSA_CLASSES - 1 && X.L > pass_rows)
                    return ctx->fail(PML_EINVAL, who + "an X of " + std::to_string(X.L) + " columns does not fit class " + std::to_string(c) + " (" + std::to_string(pass_rows) + " in its one pass)");
                const size_t npass = (size_t)std::max(1, (X.L + pass_rows - 1) / pass_rows);
                const size_t db = npass * ((size_t)Y.L + lanes - 1) * lanes * 4;
                if (db > scratch_budget)
                    return ctx->fail(PML_ENOMEM, who + "the direction words of " + std::to_string(X.L) + " x " + std::to_string(Y.L) + " cells need " + std::to_string(db) +
                                                     " bytes, the scratch budget is " + std::to_string(scratch_budget));
                MsaTask t; std::memset(&t, 0, sizeof t);
                t.x_rows = X.rows; t.y_rows = Y.rows; t.x_cnt = X.cnt; t.y_cnt = Y.cnt;
                t.LX = X.L; t.LY = Y.L; t.nX = X.n; t.nY = Y.n; t.GO = o.open * X.n * Y.n; t.GE = o.ext * X.n * Y.n; t.cls = c;
                tasks.push_back(t); tref.push_back(r); tdir.push_back(db);
            }
        const size_t nt = tasks.size();
        // sub-batches under the scratch budget, and their workgroups
        struct Sub { size_t t0, t1, b0, b1, dir; int max_LY; };
        std::vector<Sub> subs; std::vector<MsaBlock> blocks;
        for (size_t t0 = 0; t0 < nt;) {
            Sub sb{t0, t0, blocks.size(), 0, 0, 0};
            while (sb.t1 < nt && (sb.t1 == t0 || sb.dir + al(tdir[sb.t1]) <= scratch_budget)) {
                sb.dir += al(tdir[sb.t1]); sb.max_LY = std::max(sb.max_LY, tasks[sb.t1].LY); ++sb.t1;
            }
            for (size_t t = t0; t < sb.t1;) {
                const int cls = tasks[t].cls, per = MSA_THREADS / MSA_LANES[cls];
                size_t e = t;
                while (e < sb.t1 && tasks[e].cls == cls && (int)(e - t) < per) ++e;
                blocks.push_back(MsaBlock{(int)t, (int)(e - t), cls, 0});
                t = e;
            }
            sb.b1 = blocks.size();
            subs.push_back(sb); t0 = sb.t1;
        }
        size_t need_dir = 0;
        for (const Sub &sb : subs) need_dir = std::max(need_dir, sb.dir);
        if (need_dir > dir_bytes) {                                      // the last level's kernels are done: the level ended with a sync
            if (dir) bufs.drop(dir);
            MCHK(hipMalloc((void **)&dir, need_dir));
            bufs.all.push_back(dir); dir_bytes = need_dir;
        }
        // the level's arrays
        size_t off = 0;
        const size_t o_tasks = off; off += al(nt * sizeof(MsaTask));
        const size_t o_blocks = off; off += al(blocks.size() * sizeof(MsaBlock));
        const size_t o_info = off; off += al(nt * sizeof(int2));
        std::vector<size_t> o_v(nt), o_map(nt), o_lb(nt);
        for (size_t t = 0; t < nt; ++t) {
            o_v[t] = off; off += al((size_t)tasks[t].LY * 48);
            o_map[t] = off; off += al(((size_t)tasks[t].LX + tasks[t].LY) * sizeof(int2));
            o_lb[t] = off;
            if (tasks[t].LX > MSA_LANES[tasks[t].cls] * MSA_STRIP) off += al(2 * (size_t)tasks[t].LY * sizeof(int2));
        }
        char *lvl = nullptr;
        MCHK(hipMalloc((void **)&lvl, std::max<size_t>(off, 256)));
        bufs.all.push_back(lvl);
        for (const Sub &sb : subs) {
            size_t d = 0;
            for (size_t t = sb.t0; t < sb.t1; ++t) {
                tasks[t].v = (uint32_t *)(lvl + o_v[t]); tasks[t].map = (int2 *)(lvl + o_map[t]);
                tasks[t].lb = tasks[t].LX > MSA_LANES[tasks[t].cls] * MSA_STRIP ? (int2 *)(lvl + o_lb[t]) : nullptr;
                tasks[t].dir = (uint32_t *)(dir + d); d += al(tdir[t]);
            }
        }
        MCHK(hipMemcpyAsync(lvl + o_tasks, tasks.data(), nt * sizeof(MsaTask), hipMemcpyHostToDevice, ctx->stream));
        MCHK(hipMemcpyAsync(lvl + o_blocks, blocks.data(), blocks.size() * sizeof(MsaBlock), hipMemcpyHostToDevice, ctx->stream));
        MCHK(hipMemsetAsync(lvl + o_info, 0, nt * sizeof(int2), ctx->stream));
        const MsaTask *dt = (const MsaTask *)(lvl + o_tasks);
        int2 *dinfo = (int2 *)(lvl + o_info);
        for (const Sub &sb : subs) {
            // blocks index tasks from the level's first task; colv and walk take the sub-batch's range
            timed(0, [&] { launch_msa_colv(dt + sb.t0, (int)(sb.t1 - sb.t0), sb.max_LY, (const int8_t *)(base + o_tab), ctx->stream); });
            timed(1, [&] { launch_msa_dp(dt, (const MsaBlock *)(lvl + o_blocks) + sb.b0, (int)(sb.b1 - sb.b0), dinfo, ctx->stream); });
            timed(2, [&] { launch_msa_walk(dt + sb.t0, (int)(sb.t1 - sb.t0), dinfo + sb.t0, ctx->stream); });
            ctx->msa_counts[6]++;
        }
        MCHK(hipGetLastError());
        std::vector<int2> info(nt);
        MCHK(hipMemcpyAsync(info.data(), dinfo, nt * sizeof(int2), hipMemcpyDeviceToHost, ctx->stream));
        if (ctx->sync(ctx->stream)) return PML_EDEVICE;
        resolve();
        if (prev_level) { bufs.drop(prev_level); prev_level = nullptr; }
        // the merged clusters at their exact size
        size_t ob = 0; int max_Lm = 0;
        std::vector<size_t> o_or(nt), o_oc(nt);
        for (size_t t = 0; t < nt; ++t) {
            const int Lm = info[t].x;
            if (Lm < std::max(tasks[t].LX, tasks[t].LY) || Lm > tasks[t].LX + tasks[t].LY)
                return ctx->fail(PML_EDEVICE, "internal: set " + std::to_string(jobs[(size_t)tref[t].job].set) + ": a merged length of " + std::to_string(Lm));
            o_or[t] = ob; ob += al((size_t)(tasks[t].nX + tasks[t].nY) * Lm);
            o_oc[t] = ob; ob += al((size_t)Lm * 48);
            max_Lm = std::max(max_Lm, Lm);
        }
        char *out = nullptr;
        MCHK(hipMalloc((void **)&out, std::max<size_t>(ob, 256)));
        bufs.all.push_back(out);
        for (size_t t = 0; t < nt; ++t) { tasks[t].out_rows = (uint8_t *)(out + o_or[t]); tasks[t].out_cnt = (uint32_t *)(out + o_oc[t]); }
        MCHK(hipMemcpyAsync(lvl + o_tasks, tasks.data(), nt * sizeof(MsaTask), hipMemcpyHostToDevice, ctx->stream));
        timed(3, [&] { launch_msa_gather(dt, (int)nt, max_Lm, dinfo, ctx->stream); });
        MCHK(hipGetLastError());
        for (size_t t = 0; t < nt; ++t) {
            Job &j = jobs[(size_t)tref[t].job];
            const MsaMerge &m = j.plan.merges[(size_t)tref[t].merge];
            j.plan.score[(size_t)tref[t].merge] = info[t].y;
            nodes[(size_t)tref[t].job][(size_t)m.x] = Node{tasks[t].out_rows, tasks[t].out_cnt, tasks[t].nX + tasks[t].nY, info[t].x};
            ctx->msa_counts[7] += (long long)tasks[t].LX * tasks[t].LY;
            if (want_path) {
                std::vector<int2> map((size_t)info[t].x);
                MCHK(hipMemcpy(map.data(), tasks[t].map + (tasks[t].LX + tasks[t].LY - info[t].x), map.size() * sizeof(int2), hipMemcpyDeviceToHost));
                j.path.clear();
                for (const int2 &e : map) j.path.push_back((uint8_t)(e.x >= 0 && e.y >= 0 ? 0 : e.x < 0 ? 1 : 2));
            }
        }
        ctx->msa_counts[4] += (long long)nt; ctx->msa_counts[5]++;
        prev_level = lvl;
    }
    // the final clusters
    for (size_t ji = 0; ji < jobs.size(); ++ji) {
        Job &j = jobs[ji];
        const Node &root = nodes[ji][0];
        j.fin.n = root.n; j.fin.L = root.L; j.fin.rows.resize((size_t)root.n * root.L);
        if (j.plan.merges.empty()) std::memcpy(j.fin.rows.data(), j.leaves[0].rows, j.fin.rows.size());
        else MCHK(hipMemcpyAsync(j.fin.rows.data(), root.rows, j.fin.rows.size(), hipMemcpyDeviceToHost, ctx->stream));
    }
    if (ctx->sync(ctx->stream)) return PML_EDEVICE;
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

int profile_align(pml_ctx *pctx, const pml_msa_set *a, const pml_msa_set *b, const pml_msa_opts *opts, int force_class, long long *score_out, pml_msa_result *result) {
    if (result) std::memset(result, 0, sizeof *result);
    if (!pctx || !a || !b || !result) return PML_EINVAL;
    const int rc = guarded(pctx, [&](Ctx *ctx) -> int {
        if (force_class < -1 || force_class >= MSA_CLASSES) return ctx->fail(PML_EINVAL, "force_class is -1 .. 2");
        MsaOpts o; MsaProfile X, Y; std::string err;
        if (!msa_resolve(opts, o, err) || !msa_encode_profile(a, "a", X, err) || !msa_encode_profile(b, "b", Y, err)) return ctx->fail(PML_EINVAL, err);
        std::vector<Job> jobs(1);
        jobs[0].leaves.push_back({X.rows.data(), X.n, X.L});
        jobs[0].leaves.push_back({Y.rows.data(), Y.n, Y.L});
        jobs[0].plan.merges.push_back({0, 1, 1});
        if (int rc2 = msa_run(ctx, jobs, o, force_class, true)) return rc2;
        std::vector<int> members((size_t)jobs[0].fin.n);
        for (size_t r = 0; r < members.size(); ++r) members[r] = (int)r;
        jobs[0].plan.merges[0].y = X.n;                                  // as the host twin reports it: the first row of b
        if (score_out) *score_out = jobs[0].plan.score[0];
        return msa_fill_result(result, jobs[0].fin, members, jobs[0].plan, &jobs[0].path) ? ctx->fail(PML_ENOMEM, "host allocation failed") : PML_OK;
    });
    if (rc) pml_msa_result_free(result);
    return rc;
}

}  // namespace

extern "C" int pml_msa_align(pml_ctx *pctx, int nsets, const pml_msa_set *sets, const pml_msa_opts *opts, pml_msa_result *results) {
    if (results && nsets > 0) std::memset(results, 0, sizeof *results * (size_t)nsets);
    if (!pctx || nsets < 0 || (nsets > 0 && (!sets || !results))) return PML_EINVAL;
    const int rc = guarded(pctx, [&](Ctx *ctx) -> int {
        MsaOpts o; MsaInput in; std::string err;
        if (!msa_resolve(opts, o, err) || !msa_encode_sets(nsets, sets, in, err)) return ctx->fail(PML_EINVAL, err);
        if (nsets == 0) return PML_OK;
        SwOpts so = SwOpts(); so.open = o.open; so.ext = o.ext; std::memcpy(so.table, o.table, sizeof so.table);
        std::vector<Job> jobs((size_t)nsets);
        std::vector<int> len((size_t)in.set_off.back());
        for (int s = 0; s < nsets; ++s) {
            Job &j = jobs[(size_t)s];
            j.set = s;
            for (int q = in.set_off[(size_t)s]; q < in.set_off[(size_t)s + 1]; ++q) { len[(size_t)q] = in.len(q); j.leaves.push_back({in.codes.data() + in.off[(size_t)q], 1, len[(size_t)q]}); }
        }
        // the pair scores: consecutive sets share one call of the search's driver until they hold MSA_SCORE_GROUP sequences (one
        // set's launch is a few workgroups; a group scores all its sequences against each other and the sets' blocks are read)
        for (int s0 = 0; s0 < nsets;) {
            int s1 = s0 + 1;
            while (s1 < nsets && in.set_off[(size_t)s1 + 1] - in.set_off[(size_t)s0] <= MSA_SCORE_GROUP) ++s1;
            const int q0 = in.set_off[(size_t)s0], N = in.set_off[(size_t)s1] - q0;
            bool any = false;                                            // sets of one sequence need no score
            for (int s = s0; s < s1; ++s) any = any || in.set_off[(size_t)s + 1] - in.set_off[(size_t)s] >= 2;
            std::vector<int> sc;
            if (any) if (int rc2 = sw_scores_encoded(ctx, in.codes.data(), in.off.data() + q0, len.data() + q0, N, so, sc)) return rc2;
            for (int s = s0; s < s1; ++s) {
                const int a0 = in.set_off[(size_t)s] - q0, n = in.set_off[(size_t)s + 1] - in.set_off[(size_t)s];
                if (n < 2) continue;
                std::vector<long long> S((size_t)n * n);
                for (int a = 0; a < n; ++a) for (int b = 0; b < n; ++b) S[(size_t)a * n + b] = sc[(size_t)(a0 + a) * N + a0 + b];
                msa_guide_tree(n, S.data(), jobs[(size_t)s].plan.merges);
            }
            s0 = s1;
        }
        if (int rc2 = msa_run(ctx, jobs, o, -1, false)) return rc2;
        for (int s = 0; s < nsets; ++s) {
            std::vector<std::vector<int>> order;
            msa_member_orders((int)jobs[(size_t)s].leaves.size(), jobs[(size_t)s].plan.merges, order);
            if (msa_fill_result(results + s, jobs[(size_t)s].fin, order[0], jobs[(size_t)s].plan, nullptr)) return ctx->fail(PML_ENOMEM, "host allocation failed");
        }
        return PML_OK;
    });
    if (rc) for (int s = 0; s < nsets; ++s) pml_msa_result_free(results + s);
    return rc;
}

extern "C" int pml_msa_profile_align(pml_ctx *ctx, const pml_msa_set *a, const pml_msa_set *b, const pml_msa_opts *opts, long long *score_out, pml_msa_result *result) {
    return profile_align(ctx, a, b, opts, -1, score_out, result);
}

extern "C" int pml_debug_msa_profile_align(pml_ctx *ctx, const pml_msa_set *a, const pml_msa_set *b, const pml_msa_opts *opts, int force_class, long long *score_out,
                                           pml_msa_result *result) {
    return profile_align(ctx, a, b, opts, force_class, score_out, result);
}

extern "C" int pml_msa_stats(pml_ctx *ctx, long long *counts, double *total_ms) {
    if (!ctx) return PML_EINVAL;
    std::lock_guard<std::mutex> lk(ctx->c.mu);
    if (counts) for (int i = 0; i < 8; ++i) counts[i] = ctx->c.msa_counts[i];
    if (total_ms) for (int i = 0; i < 4; ++i) total_ms[i] = ctx->c.msa_ms[i];
    return PML_OK;
}
