// mash.cpp -- the device driver of the MinHash path (include/peprml.h "NeighborMasher"): pml_mash_sketch, pml_mash_dist,
// pml_mash_distances, pml_debug_mash_hashes, pml_neighbor_masher, pml_mash_stats.  The kernels are mash.hip, the rule and the Java's
// selection routines mash_host.cpp.  Genomes are worked through in sub-batches that fit the HBM budget: a sub-batch is ONE
// allocation (its bytes, one value per byte, the survivors' room of the same size, and the per-genome counters), hashed, cut,
// compacted, sorted and reduced to sketches without a host step; the host then reads two ints per genome and repeats the sub-batch
// with raised cuts where too few distinct values survived.  The sketches of a call stay resident for its pair blocks.
#include <algorithm>
#include <climits>
#include <cstring>
#include <set>

#include "../../include/peprml.h"
#include "api_types.hpp"
#include "nj.hpp"
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

// the sketches of a call in HBM: n rows of s values, and their lengths
struct Resident {
    DevBuf sk, len;
    int n = 0, s = 0;
    std::vector<int> hlen;
    uint64_t *values() const { return (uint64_t *)sk.d; }
    int *lens() const { return (int *)len.d; }
};

bool genome_ok(const pml_genome &g) {
    if (g.nrecords < 0 || (g.nrecords > 0 && (!g.records || !g.lengths))) return false;
    for (int r = 0; r < g.nrecords; ++r) if (g.lengths[r] < 0 || (g.lengths[r] > 0 && !g.records[r])) return false;
    return true;
}

size_t genome_bytes(const pml_genome &g) {
    size_t b = 0;
    for (int r = 0; r < g.nrecords; ++r) b += (size_t)g.lengths[r] + 1;
    return b;
}

// what one genome adds to a sub-batch's allocation: a byte, a value and a survivor's place per byte, the sort's double buffer
// taken as one more place, its spans, histogram and counters
size_t genome_cost(size_t bytes) {
    return bytes * (1 + 3 * sizeof(uint64_t)) + ((bytes + MASH_TILE - 1) / MASH_TILE / MASH_SPAN_TILES + 1) * sizeof(MashSpan) + MASH_BINS * sizeof(unsigned) + 64 + 3 * 256;
}

int check_ks(Ctx *ctx, int k, int s) {
    if (k < 1 || k > 32) return ctx->fail(PML_EINVAL, "k = " + std::to_string(k) + " is outside 1..32");
    if (s < 1) return ctx->fail(PML_EINVAL, "s = " + std::to_string(s) + " must be at least 1");
    return PML_OK;
}

// genomes[g0 .. g1) through the kernels; their sketches go to rows row0 + (g - g0) of R.  values_out (optional): the per-byte
// values of k_mash_hash of the (single) genome, separators included
int run_subbatch(Ctx *ctx, const pml_genome *const *genomes, int g0, int g1, int k, int s, Resident *R, int row0, std::vector<uint64_t> *values_out) {
    const int G = g1 - g0;
    std::vector<unsigned> first((size_t)G + 1, 0);
    for (int g = 0; g < G; ++g) first[(size_t)g + 1] = first[(size_t)g] + (unsigned)genome_bytes(*genomes[g0 + g]);
    const unsigned nbytes = first[(size_t)G];
    std::vector<MashSpan> spans;
    for (int g = 0; g < G; ++g)
        for (unsigned b = first[(size_t)g]; b < first[(size_t)g + 1]; b += (unsigned)MASH_TILE * MASH_SPAN_TILES)
            spans.push_back(MashSpan{b, std::min(first[(size_t)g + 1], b + (unsigned)MASH_TILE * MASH_SPAN_TILES), g});
    const int nspans = (int)spans.size();
    size_t off = 0;
    const size_t o_values = off; off += align_up((size_t)nbytes * sizeof(uint64_t), 256);
    const size_t o_comp = off; off += align_up((size_t)nbytes * sizeof(uint64_t), 256);
    const size_t o_nvalid = off; off += align_up((size_t)G * sizeof(unsigned long long), 256);
    const size_t o_hist = off; off += align_up((size_t)G * MASH_BINS * sizeof(unsigned), 256);
    const size_t zero_bytes = off - o_nvalid;          // cleared before every hashing pass
    const size_t o_count = off; off += align_up((size_t)G * sizeof(unsigned), 256);
    const size_t o_segend = off; off += align_up((size_t)G * sizeof(unsigned), 256);
    const size_t o_cut = off; off += align_up((size_t)G * sizeof(int), 256);
    const size_t o_up = off;                           // the uploaded part: min_bins, first, spans, bytes
    const size_t o_min = off; off += align_up((size_t)G * sizeof(int), 256);
    const size_t o_first = off; off += align_up(((size_t)G + 1) * sizeof(unsigned), 256);
    const size_t o_spans = off; off += align_up((size_t)nspans * sizeof(MashSpan), 256);
    const size_t o_bytes = off; off += align_up((size_t)nbytes, 256);
    DevBuf buf, tmp;
    MCHK(hipSetDevice(ctx->device));
    MCHK(hipMalloc((void **)&buf.d, std::max<size_t>(off, 256)));
    char *d = buf.d;
    std::vector<char> host(off - o_up, 0);
    int *min_bins = (int *)(host.data() + (o_min - o_up));
    for (int g = 0; g < G; ++g) min_bins[g] = ctx->mash_full_sort ? MASH_BINS : 0;
    std::memcpy(host.data() + (o_first - o_up), first.data(), first.size() * sizeof(unsigned));
    if (nspans) std::memcpy(host.data() + (o_spans - o_up), spans.data(), spans.size() * sizeof(MashSpan));
    {
        char *p = host.data() + (o_bytes - o_up);
        for (int g = 0; g < G; ++g)
            for (int r = 0; r < genomes[g0 + g]->nrecords; ++r) {
                const size_t L = (size_t)genomes[g0 + g]->lengths[r];
                if (L) std::memcpy(p, genomes[g0 + g]->records[r], L);
                p[L] = (char)MASH_SEP;
                p += L + 1;
            }
    }
    size_t tmp_bytes = 0;
    if (!values_out && nbytes) {
        MCHK(launch_mash_sort(nullptr, tmp_bytes, (const uint64_t *)(d + o_comp), (uint64_t *)(d + o_values), nbytes, G, (const unsigned *)(d + o_first),
                              (const unsigned *)(d + o_count), (unsigned *)(d + o_segend), k, ctx->stream));
        MCHK(hipMalloc((void **)&tmp.d, std::max<size_t>(tmp_bytes, 256)));
    }
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    if (ctx->profile) for (auto &e : ev) e = ctx->get_event();
    struct Back { Ctx *c; hipEvent_t *e; ~Back() { for (int i = 0; i < 4; ++i) if (e[i]) c->pool.push_back(e[i]); } } back{ctx, ev};
    std::vector<int> len((size_t)G, 0), cut((size_t)G, 0);
    for (int round = 0;; ++round) {
        if (ev[0]) hipEventRecord(ev[0], ctx->stream);
        if (round == 0) MCHK(hipMemcpyAsync(d + o_up, host.data(), host.size(), hipMemcpyHostToDevice, ctx->stream));
        else MCHK(hipMemcpyAsync(d + o_min, min_bins, (size_t)G * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
        MCHK(hipMemsetAsync(d + o_nvalid, 0, zero_bytes, ctx->stream));
        if (ev[1]) hipEventRecord(ev[1], ctx->stream);
        launch_mash_hash((const uint8_t *)(d + o_bytes), nbytes, (const MashSpan *)(d + o_spans), nspans, k, (uint64_t *)(d + o_values),
                         (unsigned long long *)(d + o_nvalid), (unsigned *)(d + o_hist), ctx->stream);
        if (nspans) ctx->mash_launches[0]++;
        if (ev[2]) hipEventRecord(ev[2], ctx->stream);
        if (values_out) {
            values_out->resize(nbytes);
            if (nbytes) MCHK(hipMemcpyAsync(values_out->data(), d + o_values, (size_t)nbytes * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
            MCHK(hipGetLastError());
            if (ctx->sync(ctx->stream)) return PML_EDEVICE;
            return PML_OK;
        }
        launch_mash_cut((const unsigned *)(d + o_hist), (const unsigned long long *)(d + o_nvalid), (const int *)(d + o_min), G, s, (int *)(d + o_cut),
                        (unsigned *)(d + o_count), ctx->stream);
        launch_mash_compact((const uint64_t *)(d + o_values), (const MashSpan *)(d + o_spans), nspans, (const unsigned *)(d + o_first), (const int *)(d + o_cut), k,
                            (uint64_t *)(d + o_comp), (unsigned *)(d + o_count), ctx->stream);
        if (nbytes)
            MCHK(launch_mash_sort(tmp.d, tmp_bytes, (const uint64_t *)(d + o_comp), (uint64_t *)(d + o_values), nbytes, G, (const unsigned *)(d + o_first),
                                  (const unsigned *)(d + o_count), (unsigned *)(d + o_segend), k, ctx->stream));
        launch_mash_unique((const uint64_t *)(d + o_values), (const unsigned *)(d + o_first), (const unsigned *)(d + o_count), G, s,
                           R->values() + (size_t)row0 * s, R->lens() + row0, ctx->stream);
        ctx->mash_launches[1]++; ctx->mash_launches[3]++;
        if (nspans) ctx->mash_launches[2]++;
        if (ev[3]) hipEventRecord(ev[3], ctx->stream);
        MCHK(hipGetLastError());
        MCHK(hipMemcpyAsync(len.data(), R->lens() + row0, (size_t)G * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        MCHK(hipMemcpyAsync(cut.data(), d + o_cut, (size_t)G * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        if (ctx->sync(ctx->stream)) return PML_EDEVICE;
        if (ev[0]) {
            float ms = 0;
            for (int i = 0; i < 3; ++i) if (hipEventElapsedTime(&ms, ev[i], ev[i + 1]) == hipSuccess) ctx->mash_ms[i] += ms;
        }
        bool again = false;
        for (int g = 0; g < G; ++g) {
            if (len[(size_t)g] < 0 || len[(size_t)g] > s || cut[(size_t)g] < 1 || cut[(size_t)g] > MASH_BINS)
                return ctx->fail(PML_EDEVICE, "internal: the selection left an impossible length or cut for genome " + std::to_string(g0 + g));
            if (len[(size_t)g] >= s || cut[(size_t)g] >= MASH_BINS) continue;
            // too few distinct values under the cut: at least twice the bins, and what the yield so far asks for
            const long long want = (long long)cut[(size_t)g] * s / std::max(len[(size_t)g], 1) + 1;
            min_bins[g] = (int)std::min<long long>(MASH_BINS, std::max<long long>(2ll * cut[(size_t)g], want));
            again = true;
        }
        if (!again) break;
        ctx->mash_repeats++;
        if (round > MASH_BIN_BITS + 1) return ctx->fail(PML_EDEVICE, "internal: the cut did not reach every bin");
    }
    for (int g = 0; g < G; ++g) R->hlen[(size_t)(row0 + g)] = len[(size_t)g];
    return PML_OK;
}

int resident_alloc(Ctx *ctx, Resident &R, int n, int s) {
    R.n = n; R.s = s; R.hlen.assign((size_t)n, 0);
    MCHK(hipSetDevice(ctx->device));
    MCHK(hipMalloc((void **)&R.sk.d, std::max<size_t>((size_t)n * s * sizeof(uint64_t), 256)));
    MCHK(hipMalloc((void **)&R.len.d, std::max<size_t>((size_t)n * sizeof(int), 256)));
    return PML_OK;
}

// every genome's sketch into R (allocated here), sub-batched under the budget
int sketch_all(Ctx *ctx, const std::vector<const pml_genome *> &genomes, int k, int s, Resident &R) {
    const int n = (int)genomes.size();
    for (int g = 0; g < n; ++g) if (!genomes[(size_t)g] || !genome_ok(*genomes[(size_t)g])) return ctx->fail(PML_EINVAL, "genome " + std::to_string(g) + " is malformed");
    if (int rc = resident_alloc(ctx, R, n, s)) return rc;
    const size_t budget = trim_hbm_budget(ctx);
    for (int g0 = 0; g0 < n;) {
        size_t need = TRIM_BATCH_SLACK, bytes = 0; int g1 = g0;
        while (g1 < n) {
            const size_t b = genome_bytes(*genomes[(size_t)g1]), c = genome_cost(b);
            if (need + c > budget || bytes + b >= ((size_t)1 << 31)) break;
            need += c; bytes += b; ++g1;
        }
        if (g1 == g0) {
            const size_t b = genome_bytes(*genomes[(size_t)g0]), c = TRIM_BATCH_SLACK + genome_cost(b);
            return ctx->fail(PML_ENOMEM, "genome " + std::to_string(g0) + " (" + std::to_string(b) + " bytes with its separators) needs " +
                                             std::to_string((c + ((size_t)1 << 20) - 1) >> 20) + " MiB of HBM for its bytes, values and survivors, the budget is " +
                                             std::to_string(budget >> 20) + " MiB; a genome of 2^31 bytes or more does not fit at all");
        }
        if (int rc = run_subbatch(ctx, genomes.data(), g0, g1, k, s, &R, g0, nullptr)) return rc;
        g0 = g1;
    }
    return PML_OK;
}

// (common, denom) of rows x cols of R, one launch per block of rows; out is rows.size() x cols.size(), row major
int pair_block(Ctx *ctx, const Resident &R, const std::vector<int> &rows, const std::vector<int> &cols, std::vector<int> &common, std::vector<int> &denom) {
    const size_t nr = rows.size(), nc = cols.size();
    common.assign(nr * nc, 0); denom.assign(nr * nc, 0);
    if (!nr || !nc) return PML_OK;
    const size_t budget = trim_hbm_budget(ctx);
    const size_t fixed = align_up((nr + nc) * sizeof(int), 256) + 256;
    size_t block = budget > fixed ? (budget - fixed) / (nc * sizeof(int2)) : 0;
    block = std::min<size_t>(std::min<size_t>(block, 65535), nr);
    if (block < 1) return ctx->fail(PML_ENOMEM, "one row of " + std::to_string(nc) + " pair results does not fit the HBM budget of " + std::to_string(budget >> 20) + " MiB");
    DevBuf buf;
    MCHK(hipSetDevice(ctx->device));
    const size_t o_cols = align_up(nr * sizeof(int), 256), o_out = o_cols + align_up(nc * sizeof(int), 256);
    MCHK(hipMalloc((void **)&buf.d, o_out + block * nc * sizeof(int2)));
    MCHK(hipMemcpyAsync(buf.d, rows.data(), nr * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    MCHK(hipMemcpyAsync(buf.d + o_cols, cols.data(), nc * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    std::vector<int2> host(block * nc);
    for (size_t r0 = 0; r0 < nr; r0 += block) {
        const size_t m = std::min(block, nr - r0);
        hipEvent_t e0 = nullptr, e1 = nullptr;
        if (ctx->profile) { e0 = ctx->get_event(); e1 = ctx->get_event(); hipEventRecord(e0, ctx->stream); }
        launch_mash_pairs(R.values(), R.lens(), (const int *)buf.d + r0, (int)m, (const int *)(buf.d + o_cols), (int)nc, R.s, (int2 *)(buf.d + o_out), ctx->stream);
        if (e1) hipEventRecord(e1, ctx->stream);
        ctx->mash_launches[4]++;
        hipError_t err = hipGetLastError();
        if (err == hipSuccess) err = hipMemcpyAsync(host.data(), buf.d + o_out, m * nc * sizeof(int2), hipMemcpyDeviceToHost, ctx->stream);
        const int bad = err != hipSuccess ? ctx->fail(PML_EDEVICE, std::string("k_mash_pairs: ") + hipGetErrorString(err)) : ctx->sync(ctx->stream) ? PML_EDEVICE : 0;
        if (e0) {
            float ms = 0;
            if (!bad && hipEventElapsedTime(&ms, e0, e1) == hipSuccess) ctx->mash_ms[3] += ms;
            ctx->pool.push_back(e0); ctx->pool.push_back(e1);
        }
        if (bad) return bad;
        for (size_t i = 0; i < m * nc; ++i) { common[r0 * nc + i] = host[i].x; denom[r0 * nc + i] = host[i].y; }
    }
    return PML_OK;
}

void fill_distances(const std::vector<int> &common, const std::vector<int> &denom, int k, int digits, int *c_out, int *d_out, double *dist_out) {
    for (size_t i = 0; i < common.size(); ++i) {
        if (c_out) c_out[i] = common[i];
        if (d_out) d_out[i] = denom[i];
        if (dist_out) dist_out[i] = mash_round_digits(mash_distance_of(common[i], denom[i], k), digits);
    }
}

template <class F> int guarded(pml_ctx *pctx, F f) {
    std::lock_guard<std::mutex> lk(pctx->c.mu);
    pml_fpguard fpg;
    pml_drop_worker_caches(pctx);
    try { return f(&pctx->c); }
    catch (const std::bad_alloc &) { return pctx->c.fail(PML_ENOMEM, "host allocation failed"); }
    catch (const std::exception &e) { return pctx->c.fail(PML_EINVAL, e.what()); }
}

char *dup_string(const std::string &s) { char *p = (char *)std::malloc(s.size() + 1); if (p) std::memcpy(p, s.c_str(), s.size() + 1); return p; }

int check_names(Ctx *ctx, const char *what, int n, const char *const *names) {
    if (n < 1 || !names) return ctx->fail(PML_EINVAL, std::string("the ") + what + " name list is empty");
    std::set<std::string> seen;
    for (int i = 0; i < n; ++i) {
        if (!names[i]) return ctx->fail(PML_EINVAL, std::string("a null ") + what + " name");
        if (!seen.insert(names[i]).second) return ctx->fail(PML_EINVAL, std::string("the ") + what + " taxon name '" + names[i] + "' occurs twice");
    }
    return PML_OK;
}

// NeighborMasher.run() :112-195
int neighbor_masher(Ctx *ctx, const pml_neighbor_masher_opts &o, pml_neighbor_masher_result *res) {
    if (int rc = check_ks(ctx, o.k, o.s)) return rc;
    if (int rc = check_names(ctx, "ingroup", o.n_ingroup, o.ingroup_names)) return rc;
    const bool expand = o.expand_ingroup > o.n_ingroup;                       // :116
    const bool need_pool = expand || !o.ingroup_only;
    if (o.n_pool < 0 || (need_pool && o.n_pool < 1)) return ctx->fail(PML_EINVAL, "the pool name list is empty");
    if (o.n_pool > 0) if (int rc = check_names(ctx, "pool", o.n_pool, o.pool_names)) return rc;
    if (!o.ingroup || (o.n_pool > 0 && !o.pool)) return PML_EINVAL;
    const int NI = o.n_ingroup, NP = o.n_pool, N = NI + NP;
    std::vector<const pml_genome *> genomes;
    std::vector<std::string> names;
    for (int i = 0; i < NI; ++i) { genomes.push_back(&o.ingroup[i]); names.push_back(o.ingroup_names[i]); }
    for (int p = 0; p < NP; ++p) { genomes.push_back(&o.pool[p]); names.push_back(o.pool_names[p]); }
    Resident R;
    if (int rc = sketch_all(ctx, genomes, o.k, o.s, R)) return rc;
    for (int g = 0; g < N; ++g)
        if (R.hlen[(size_t)g] == 0)
            return ctx->fail(PML_EINVAL, std::string(g < NI ? "ingroup" : "pool") + " genome '" + names[(size_t)g] + "' has no valid window of " + std::to_string(o.k) +
                                             " bases: its sketch is empty");
    std::vector<int> pool_idx((size_t)NP), ingroup((size_t)NI);
    for (int p = 0; p < NP; ++p) pool_idx[(size_t)p] = NI + p;
    for (int i = 0; i < NI; ++i) ingroup[(size_t)i] = i;
    std::vector<int> common, denom;
    auto distances = [&](const std::vector<int> &rows, const std::vector<int> &cols, std::vector<double> &d) -> int {
        if (int rc = pair_block(ctx, R, rows, cols, common, denom)) return rc;
        d.resize(common.size());
        fill_distances(common, denom, o.k, o.digits, nullptr, nullptr, d.data());
        return PML_OK;
    };
    if (expand) {                                                             // expandIngroup :281-324
        std::set<std::string> original(names.begin(), names.begin() + NI);
        std::vector<unsigned char> is_in((size_t)NP);
        for (int p = 0; p < NP; ++p) is_in[(size_t)p] = original.count(names[(size_t)(NI + p)]) ? 1 : 0;
        std::vector<double> d;
        if (int rc = distances(pool_idx, ingroup, d)) return rc;
        std::vector<int> added;
        mash_expand_ingroup(NI, NP, d.data(), is_in.data(), o.expand_ingroup, added);
        for (int p : added) ingroup.push_back(NI + p);
    }
    const int F = (int)ingroup.size();
    std::vector<int> outgroup;                                                // pool indices
    std::vector<double> cand;
    double mean = std::nan(""), sd = std::nan(""), mx = std::nan("");
    std::vector<double> dff;                                                  // final ingroup x final ingroup
    if (int rc = distances(ingroup, ingroup, dff)) return rc;
    if (!o.ingroup_only) {                                                    // :148-164
        std::vector<double> pairs;                                            // getIngroupPairDistances :855-867
        for (int i = 0; i < F; ++i) for (int j = i + 1; j < F; ++j) pairs.push_back(dff[(size_t)i * F + j]);
        mash_pair_stats(pairs, mean, sd, mx);
        std::vector<double> dpf;
        if (int rc = distances(pool_idx, ingroup, dpf)) return rc;
        cand.resize((size_t)NP);
        for (int p = 0; p < NP; ++p) cand[(size_t)p] = mash_candidate_max(dpf.data() + (size_t)p * F, F);     // :738-783
        mash_select_outgroup(NP, cand.data(), mx, sd, o.outgroup_count, outgroup);
    }
    // the taxa of buildRootedTree :623-635: the outgroups first, then the ingroup
    std::vector<int> taxa;
    for (int p : outgroup) taxa.push_back(NI + p);
    for (int g : ingroup) taxa.push_back(g);
    const int T = (int)taxa.size();
    std::vector<int> tc, td;
    if (int rc = pair_block(ctx, R, taxa, taxa, tc, td)) return rc;
    std::vector<double> dist((size_t)T * T);
    fill_distances(tc, td, o.k, o.digits, nullptr, nullptr, dist.data());
    for (int i = 0; i < T; ++i) {                                             // buildNJTreeOfTaxa :654-673: the upper triangle, mirrored
        dist[(size_t)i * T + i] = 0;
        for (int j = i + 1; j < T; ++j) dist[(size_t)j * T + i] = dist[(size_t)i * T + j];
    }
    std::string ingroup_tree, rooted_tree, err;
    const int NO = (int)outgroup.size();
    if (!o.outgroup_only && o.expand_ingroup > 3 && F >= 4) {                 // :128
        std::vector<std::string> nm;
        std::vector<double> m((size_t)F * F);
        for (int i = 0; i < F; ++i) { nm.push_back(names[(size_t)ingroup[(size_t)i]]); for (int j = 0; j < F; ++j) m[(size_t)i * F + j] = dist[(size_t)(NO + i) * T + NO + j]; }
        if (!nj_tree_string(F, nm, m.data(), NJ_DISTANCE, ingroup_tree, err)) return ctx->fail(PML_EINVAL, "ingroup tree: " + err);
    }
    if (!o.ingroup_only && !o.outgroup_only && o.expand_ingroup + NO > 3 && T >= 4) {      // :175-181
        std::vector<std::string> nm;
        for (int g : taxa) nm.push_back(names[(size_t)g]);
        if (!nj_tree_string(T, nm, dist.data(), NJ_DISTANCE, rooted_tree, err)) return ctx->fail(PML_EINVAL, "ingroup and outgroup tree: " + err);
    }
    res->n_ingroup = F; res->n_outgroup = NO; res->n_pool = NP; res->n_taxa = T;
    res->mean = mean; res->sd = sd; res->max = mx;
    res->ingroup = (int *)std::malloc(sizeof(int) * (size_t)std::max(F, 1));
    res->outgroup = (int *)std::malloc(sizeof(int) * (size_t)std::max(NO, 1));
    res->taxa = (int *)std::malloc(sizeof(int) * (size_t)std::max(T, 1));
    res->distance = (double *)std::malloc(sizeof(double) * (size_t)std::max(T * T, 1));
    res->common = (int *)std::malloc(sizeof(int) * (size_t)std::max(T * T, 1));
    res->denom = (int *)std::malloc(sizeof(int) * (size_t)std::max(T * T, 1));
    res->sketch_len = (int *)std::malloc(sizeof(int) * (size_t)N);
    if (!cand.empty()) res->candidate_distance = (double *)std::malloc(sizeof(double) * (size_t)NP);
    if (!ingroup_tree.empty()) res->ingroup_tree = dup_string(ingroup_tree);
    if (!rooted_tree.empty()) res->rooted_tree = dup_string(rooted_tree);
    if (!res->ingroup || !res->outgroup || !res->taxa || !res->distance || !res->common || !res->denom || !res->sketch_len || (!cand.empty() && !res->candidate_distance) ||
        (!ingroup_tree.empty() && !res->ingroup_tree) || (!rooted_tree.empty() && !res->rooted_tree))
        return ctx->fail(PML_ENOMEM, "host allocation failed");
    std::copy(ingroup.begin(), ingroup.end(), res->ingroup);
    std::copy(outgroup.begin(), outgroup.end(), res->outgroup);
    std::copy(taxa.begin(), taxa.end(), res->taxa);
    std::copy(dist.begin(), dist.end(), res->distance);
    std::copy(tc.begin(), tc.end(), res->common);
    std::copy(td.begin(), td.end(), res->denom);
    std::copy(R.hlen.begin(), R.hlen.end(), res->sketch_len);
    if (!cand.empty()) std::copy(cand.begin(), cand.end(), res->candidate_distance);
    return PML_OK;
}

}  // namespace

extern "C" int pml_mash_sketch(pml_ctx *pctx, int ngenomes, const pml_genome *genomes, int k, int s, unsigned long long *values_out, int *len_out) {
    if (!pctx || ngenomes < 1 || !genomes || !values_out || !len_out) return PML_EINVAL;
    return guarded(pctx, [&](Ctx *ctx) -> int {
        if (int rc = check_ks(ctx, k, s)) return rc;
        std::vector<const pml_genome *> gs;
        for (int g = 0; g < ngenomes; ++g) gs.push_back(&genomes[g]);
        Resident R;
        if (int rc = sketch_all(ctx, gs, k, s, R)) return rc;
        MCHK(hipMemcpyAsync(values_out, R.values(), (size_t)ngenomes * s * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
        if (ctx->sync(ctx->stream)) return PML_EDEVICE;
        for (int g = 0; g < ngenomes; ++g) {                                  // what lies behind a sketch's end is not the caller's business
            len_out[g] = R.hlen[(size_t)g];
            std::fill(values_out + (size_t)g * s + len_out[g], values_out + (size_t)(g + 1) * s, 0ull);
        }
        return PML_OK;
    });
}

extern "C" int pml_debug_mash_hashes(pml_ctx *pctx, const pml_genome *genome, int k, unsigned long long *values_out) {
    if (!pctx || !genome || !values_out) return PML_EINVAL;
    return guarded(pctx, [&](Ctx *ctx) -> int {
        if (int rc = check_ks(ctx, k, 1)) return rc;
        if (!genome_ok(*genome)) return ctx->fail(PML_EINVAL, "the genome is malformed");
        const size_t b = genome_bytes(*genome);
        if (b >= ((size_t)1 << 31) || TRIM_BATCH_SLACK + genome_cost(b) > trim_hbm_budget(ctx)) return ctx->fail(PML_ENOMEM, "the genome does not fit the HBM budget");
        std::vector<uint64_t> v;
        if (int rc = run_subbatch(ctx, &genome, 0, 1, k, 1, nullptr, 0, &v)) return rc;
        size_t at = 0, out = 0;
        for (int r = 0; r < genome->nrecords; ++r) {                          // the separators' entries are dropped
            for (long long i = 0; i < genome->lengths[r]; ++i) values_out[out++] = v[at + (size_t)i];
            at += (size_t)genome->lengths[r] + 1;
        }
        return PML_OK;
    });
}

extern "C" int pml_mash_dist(pml_ctx *pctx, int na, const unsigned long long *a_values, const int *a_len, int nb, const unsigned long long *b_values, const int *b_len,
                             int k, int s, int digits, int *common_out, int *denom_out, double *distance_out) {
    if (!pctx || na < 1 || nb < 1 || !a_values || !a_len || !b_values || !b_len) return PML_EINVAL;
    return guarded(pctx, [&](Ctx *ctx) -> int {
        if (int rc = check_ks(ctx, k, s)) return rc;
        const int n = na + nb;
        std::vector<uint64_t> host((size_t)n * s, 0);
        Resident R;
        if (int rc = resident_alloc(ctx, R, n, s)) return rc;
        for (int g = 0; g < n; ++g) {
            const unsigned long long *v = g < na ? a_values + (size_t)g * s : b_values + (size_t)(g - na) * s;
            const int len = g < na ? a_len[g] : b_len[g - na];
            if (len < 0 || len > s) return ctx->fail(PML_EINVAL, "sketch " + std::to_string(g) + " has length " + std::to_string(len) + ", outside 0.." + std::to_string(s));
            for (int i = 0; i < len; ++i) {
                if (i && v[i] <= v[i - 1]) return ctx->fail(PML_EINVAL, "sketch " + std::to_string(g) + " is not ascending and distinct at " + std::to_string(i));
                host[(size_t)g * s + i] = v[i];
            }
            R.hlen[(size_t)g] = len;
        }
        MCHK(hipMemcpyAsync(R.values(), host.data(), host.size() * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
        MCHK(hipMemcpyAsync(R.lens(), R.hlen.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
        std::vector<int> rows, cols, common, denom;
        for (int i = 0; i < na; ++i) rows.push_back(i);
        for (int j = 0; j < nb; ++j) cols.push_back(na + j);
        if (int rc = pair_block(ctx, R, rows, cols, common, denom)) return rc;
        fill_distances(common, denom, k, digits, common_out, denom_out, distance_out);
        return PML_OK;
    });
}

extern "C" int pml_mash_distances(pml_ctx *pctx, int na, const pml_genome *a, int nb, const pml_genome *b, int k, int s, int digits, int *common_out, int *denom_out,
                                  double *distance_out) {
    if (!pctx || na < 1 || nb < 1 || !a || !b) return PML_EINVAL;
    return guarded(pctx, [&](Ctx *ctx) -> int {
        if (int rc = check_ks(ctx, k, s)) return rc;
        std::vector<const pml_genome *> gs;
        std::vector<int> rows, cols, common, denom;
        for (int i = 0; i < na; ++i) { gs.push_back(&a[i]); rows.push_back(i); }
        for (int j = 0; j < nb; ++j) { gs.push_back(&b[j]); cols.push_back(na + j); }
        Resident R;
        if (int rc = sketch_all(ctx, gs, k, s, R)) return rc;
        if (int rc = pair_block(ctx, R, rows, cols, common, denom)) return rc;
        fill_distances(common, denom, k, digits, common_out, denom_out, distance_out);
        return PML_OK;
    });
}

extern "C" void pml_neighbor_masher_result_free(pml_neighbor_masher_result *r) {
    if (!r) return;
    std::free(r->ingroup); std::free(r->outgroup); std::free(r->taxa); std::free(r->distance); std::free(r->common); std::free(r->denom);
    std::free(r->sketch_len); std::free(r->candidate_distance); std::free(r->ingroup_tree); std::free(r->rooted_tree);
    std::memset(r, 0, sizeof *r);
}

extern "C" int pml_neighbor_masher(pml_ctx *pctx, const pml_neighbor_masher_opts *opts, pml_neighbor_masher_result *result) {
    if (result) std::memset(result, 0, sizeof *result);
    if (!pctx || !opts || !result) return PML_EINVAL;
    const int rc = guarded(pctx, [&](Ctx *ctx) -> int { return neighbor_masher(ctx, *opts, result); });
    if (rc) pml_neighbor_masher_result_free(result);
    return rc;
}

extern "C" int pml_mash_stats(pml_ctx *ctx, long long *launches, double *total_ms, long long *repeats) {
    if (!ctx) return PML_EINVAL;
    std::lock_guard<std::mutex> lk(ctx->c.mu);
    if (launches) for (int i = 0; i < 5; ++i) launches[i] = ctx->c.mash_launches[i];
    if (total_ms) for (int i = 0; i < 4; ++i) total_ms[i] = ctx->c.mash_ms[i];
    if (repeats) *repeats = ctx->c.mash_repeats;
    return PML_OK;
}

extern "C" int pml_debug_mash_full_sort(pml_ctx *ctx, int on) {
    if (!ctx) return PML_EINVAL;
    std::lock_guard<std::mutex> lk(ctx->c.mu);
    ctx->c.mash_full_sort = on != 0;
    return PML_OK;
}
