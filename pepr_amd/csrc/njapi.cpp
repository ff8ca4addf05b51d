// njapi.cpp -- the device-backed half of the `nj` C ABI (include/peprml.h): pair scores through k_pairscore / k_pairscore_sum
// (pairscore.hip), trees through nj.cpp.  Every gene of a call is encoded into 24-code bytes (its own alphabet: the engine's
// resident code matrix merges X, gap and unknown), scored once, and kept as an integer matrix in HBM for the call; the code
// bytes travel in sub-batches sized by free HBM and are not kept.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <unordered_map>

#include "../../include/peprml.h"
#include "api_types.hpp"
#include "nj.hpp"

using namespace pml;

namespace {
char *dup_cstr(const std::string &s) { char *p = (char *)std::malloc(s.size() + 1); if (p) std::memcpy(p, s.c_str(), s.size() + 1); return p; }

#define NJCHK(expr)                                                                                                   \
    do { hipError_t e_ = (expr);                                                                                      \
         if (e_ != hipSuccess) return ctx->fail(PML_EDEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); } while (0)

// the per-gene score matrices of one call, resident in HBM until the call returns
struct PairScores {
    Ctx *ctx = nullptr;
    char *d_res = nullptr;                 // table + the genes' ntax x ntax int64 matrices
    char *d_codes = nullptr;               // one sub-batch of code bytes + its requests
    std::vector<size_t> mat_off; std::vector<int> ntax; size_t res_bytes = 0;
    long long *mat(int g) const { return (long long *)(d_res + mat_off[g]); }
    ~PairScores() { if (d_codes) hipFree(d_codes); if (d_res) hipFree(d_res); }

    // gap_row: every gene gets one more row of gap codes behind its taxa (index ntax), the row a taxon the gene lacks stands for
    int run(int ngenes, const pml_alignment *genes, const int *table576, int chunk_sites, bool gap_row = false) {
        if (chunk_sites == 0) chunk_sites = PS_CHUNK_DEFAULT;
        if (chunk_sites < 16 || chunk_sites % 16 || chunk_sites > PS_MAX_CHUNK) return ctx->fail(PML_EINVAL, "chunk_sites must be a multiple of 16, at most 2^20");
        int tab[NJ_CODES * NJ_CODES];
        if (table576) std::memcpy(tab, table576, sizeof tab); else blosum62_as_loaded(tab);
        int8_t tab8[PS_CODES * PS_TSTRIDE] = {0};
        for (int i = 0; i < NJ_CODES; ++i)
            for (int j = 0; j < NJ_CODES; ++j) {
                const int v = tab[i * NJ_CODES + j];
                if (v < -128 || v > 127) return ctx->fail(PML_EINVAL, "score table entry [" + std::to_string(i) + "][" + std::to_string(j) + "] = " + std::to_string(v) + " is outside [-128, 127]");
                tab8[i * PS_TSTRIDE + j] = (int8_t)v;
            }
        // layout: per-gene matrices behind the table; per-gene code bytes (rows of ld = nsites rounded up to 16)
        std::vector<size_t> code_bytes((size_t)ngenes), ld((size_t)ngenes);
        mat_off.resize((size_t)ngenes); ntax.resize((size_t)ngenes);
        size_t off = align_up(sizeof tab8, 256);
        for (int g = 0; g < ngenes; ++g) {
            const pml_alignment &A = genes[g];
            if (!A.names || !A.rows || A.ntax <= 0 || A.nsites <= 0) return ctx->fail(PML_EINVAL, "bad alignment (gene " + std::to_string(g) + ")");
            // a launch has (tiles of 16 taxa)^2 workgroups of 256 threads in x and HIP caps a grid dimension at 2^32 threads: 4096 tiles
            if (A.ntax + (gap_row ? 1 : 0) > PS_TILE * 4096)
                return ctx->fail(PML_EINVAL, "gene " + std::to_string(g) + " has " + std::to_string(A.ntax) + " taxa: a pair-score launch takes at most " +
                                                 std::to_string(PS_TILE * 4096 - (gap_row ? 1 : 0)) + (gap_row ? " with a table whose gap line is not zero" : ""));
            for (int i = 0; i < A.ntax; ++i) if (!A.names[i] || !A.rows[i]) return ctx->fail(PML_EINVAL, "bad alignment (gene " + std::to_string(g) + ")");
            ntax[g] = A.ntax + (gap_row ? 1 : 0); ld[g] = align_up((size_t)A.nsites, 16); code_bytes[g] = align_up((size_t)ntax[g] * ld[g], 256);
            mat_off[g] = off; off += align_up((size_t)ntax[g] * ntax[g] * sizeof(long long), 256);
        }
        res_bytes = off;
        NJCHK(hipSetDevice(ctx->device));
        NJCHK(hipMalloc((void **)&d_res, res_bytes));
        // sub-batches of code bytes by free HBM (PML_HBM_BUDGET_MB as in the jackknife); a gene larger than the budget goes alone
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = (size_t)1 << 40;
        size_t budget = (size_t)(0.85 * (double)free_b);
        if (const char *e = std::getenv("PML_HBM_BUDGET_MB")) budget = (size_t)std::atoll(e) << 20;
        std::vector<std::pair<int, int>> parts; size_t max_part = 0;
        for (int begin = 0; begin < ngenes;) {
            size_t used = 0; int end = begin;
            while (end < ngenes && end - begin < 65535) { if (end > begin && used + code_bytes[end] > budget) break; used += code_bytes[end]; ++end; }
            parts.push_back({begin, end}); max_part = std::max(max_part, used + align_up((size_t)(end - begin) * sizeof(PairScoreReq), 256));
            begin = end;
        }
        NJCHK(hipMalloc((void **)&d_codes, max_part));
        NJCHK(hipMemcpyAsync(d_res, tab8, sizeof tab8, hipMemcpyHostToDevice, ctx->stream));
        NJCHK(hipMemsetAsync(d_res + align_up(sizeof tab8, 256), 0, res_bytes - align_up(sizeof tab8, 256), ctx->stream));      // on the call's stream, in front of its launches
        std::vector<uint8_t> host;
        for (auto &part : parts) {
            const int n = part.second - part.first;
            const size_t req_bytes = align_up((size_t)n * sizeof(PairScoreReq), 256);
            size_t bytes = req_bytes; for (int g = part.first; g < part.second; ++g) bytes += code_bytes[g];
            host.assign(bytes, (uint8_t)NJ_GAP);
            PairScoreReq *reqs = (PairScoreReq *)host.data();
            size_t o = req_bytes; int max_ntax = 0, max_nsites = 0; double cells = 0;
            for (int g = part.first; g < part.second; ++g) {
                const pml_alignment &A = genes[g];
                for (int i = 0; i < A.ntax; ++i) {
                    if ((int)strnlen(A.rows[i], (size_t)A.nsites) < A.nsites) return ctx->fail(PML_EINVAL, "row shorter than nsites (gene " + std::to_string(g) + ", taxon '" + A.names[i] + "')");
                    int col = 0, byte = 0;
                    if (nj_encode24(A.rows[i], A.nsites, host.data() + o + (size_t)i * ld[g], &col, &byte)) {
                        char hex[8]; std::snprintf(hex, sizeof hex, "0x%02x", byte);
                        return ctx->fail(PML_EPARSE, "gene " + std::to_string(g) + ", taxon '" + A.names[i] + "', column " + std::to_string(col) + ": byte " + hex +
                                                         (byte >= 33 && byte < 127 ? std::string(" ('") + (char)byte + "')" : std::string()) +
                                                         " is not one of the 24 residue codes (the reference drops it and shifts the row)");
                    }
                }
                reqs[g - part.first] = PairScoreReq{(const uint8_t *)(d_codes + o), mat(g), ntax[g], A.nsites, (int)ld[g]};      // the gap row is the staging buffer's fill
                max_ntax = std::max(max_ntax, ntax[g]); max_nsites = std::max(max_nsites, A.nsites); cells += (double)A.ntax * A.nsites;
                o += code_bytes[g];
            }
            if (((size_t)max_nsites + chunk_sites - 1) / chunk_sites > 65535) return ctx->fail(PML_EINVAL, "alignment too long for chunk_sites");
            NJCHK(hipMemcpyAsync(d_codes, host.data(), bytes, hipMemcpyHostToDevice, ctx->stream));
            ctx->tic(K_PAIRSCORE, cells);
            launch_pairscore((const PairScoreReq *)d_codes, n, max_ntax, max_nsites, chunk_sites, (const int8_t *)d_res, ctx->stream);
            ctx->toc();
            NJCHK(hipGetLastError());
            if (ctx->sync(ctx->stream)) return PML_EDEVICE;           // the staging vector and d_codes are reused by the next part
            ctx->resolve_events();
        }
        return PML_OK;
    }
    int read(int g, std::vector<long long> &out) const {
        Ctx *ctx = this->ctx;
        out.resize((size_t)ntax[g] * ntax[g]);
        NJCHK(hipMemcpy(out.data(), mat(g), out.size() * sizeof(long long), hipMemcpyDeviceToHost));
        return PML_OK;
    }
};

// one replicate: its sorted taxon union and the integer score sums of its genes over that union
struct Replicate { std::vector<std::string> names; std::vector<long long> sums; };

// every selection's matrix: one k_pairscore pass over all genes, one k_pairscore_sum launch, one copy back
int replicate_scores(Ctx *ctx, int ngenes, const pml_alignment *genes, const std::vector<std::vector<int>> &sels, const int *table576,
                     std::vector<Replicate> &reps) {
    const int nrep = (int)sels.size();
    if (nrep > 65535) return ctx->fail(PML_EINVAL, "at most 65535 replicates per call");
    // A taxon a gene lacks is a row of '?' in the concatenation.  With a gap row and column of zeros (BLOSUM62 as loaded) that
    // row scores 0 and the kernel's loc = -1 serves; any other table gets a real gap row per gene, and absent taxa point at it.
    bool gap_row = false;
    for (int c = 0; table576 && c < NJ_CODES; ++c) gap_row = gap_row || table576[NJ_GAP * NJ_CODES + c] != 0 || table576[c * NJ_CODES + NJ_GAP] != 0;
    PairScores ps; ps.ctx = ctx;
    if (int rc = ps.run(ngenes, genes, table576, 0, gap_row)) return rc;
    std::vector<std::unordered_map<std::string, int>> index((size_t)ngenes);
    for (int g = 0; g < ngenes; ++g) for (int i = 0; i < genes[g].ntax; ++i) index[g][genes[g].names[i]] = i;      // a repeated name: the last row, as pml_concatenate
    reps.assign((size_t)nrep, Replicate());
    // host image: requests | S pointers | gene_ntax | per replicate sel and loc; then the outputs
    std::vector<size_t> o_sel((size_t)nrep), o_loc((size_t)nrep), o_out((size_t)nrep);
    size_t off = align_up((size_t)nrep * sizeof(PairSumReq), 256);
    const size_t o_S = off; off += align_up((size_t)ngenes * sizeof(long long *), 256);
    const size_t o_nt = off; off += align_up((size_t)ngenes * sizeof(int), 256);
    int max_nu = 0;
    for (int r = 0; r < nrep; ++r) {
        std::set<std::string> uni;                     // std::set order == Arrays.sort for ASCII names (MSAConcatenator)
        for (int g : sels[r]) {
            if (g < 0 || g >= ngenes) return ctx->fail(PML_EINVAL, "gene index out of range");
            for (int i = 0; i < genes[g].ntax; ++i) uni.insert(genes[g].names[i]);
        }
        reps[r].names.assign(uni.begin(), uni.end());
        const size_t nu = reps[r].names.size(), k = sels[r].size();
        max_nu = std::max(max_nu, (int)nu);
        o_sel[r] = off; off += align_up(k * sizeof(int), 256);
        o_loc[r] = off; off += align_up(k * nu * sizeof(int), 256);
    }
    const size_t in_bytes = off;
    for (int r = 0; r < nrep; ++r) { o_out[r] = off; off += align_up(reps[r].names.size() * reps[r].names.size() * sizeof(long long), 256); }
    char *d = nullptr;
    NJCHK(hipMalloc((void **)&d, off));
    struct Drop { char *p; ~Drop() { hipFree(p); } } drop{d};
    std::vector<char> host(in_bytes, 0);
    for (int g = 0; g < ngenes; ++g) { ((const long long **)(host.data() + o_S))[g] = ps.mat(g); ((int *)(host.data() + o_nt))[g] = ps.ntax[g]; }
    for (int r = 0; r < nrep; ++r) {
        const int nu = (int)reps[r].names.size(), k = (int)sels[r].size();
        int *sel = (int *)(host.data() + o_sel[r]), *loc = (int *)(host.data() + o_loc[r]);
        for (int s = 0; s < k; ++s) {
            const int g = sels[r][s];
            sel[s] = g;
            for (int t = 0; t < nu; ++t) { auto it = index[g].find(reps[r].names[t]); loc[(size_t)s * nu + t] = it != index[g].end() ? it->second : gap_row ? genes[g].ntax : -1; }
        }
        ((PairSumReq *)host.data())[r] = PairSumReq{(const int *)(d + o_sel[r]), (const int *)(d + o_loc[r]), (long long *)(d + o_out[r]), k, nu};
    }
    NJCHK(hipMemcpyAsync(d, host.data(), in_bytes, hipMemcpyHostToDevice, ctx->stream));
    hipEvent_t ev_a = nullptr, ev_b = nullptr;         // profile mode: the launch's HIP-event time (pml_pairscore_sum_stats)
    if (ctx->profile) { ev_a = ctx->get_event(); ev_b = ctx->get_event(); hipEventRecord(ev_a, ctx->stream); }
    launch_pairscore_sum((const PairSumReq *)d, nrep, max_nu, (const long long *const *)(d + o_S), (const int *)(d + o_nt), ctx->stream);
    if (ev_b) hipEventRecord(ev_b, ctx->stream);
    struct Back { Ctx *c; hipEvent_t a, b; ~Back() { if (a) c->pool.push_back(a); if (b) c->pool.push_back(b); } } back_ev{ctx, ev_a, ev_b};
    ctx->pairsum_launches++;
    NJCHK(hipGetLastError());
    std::vector<char> back(off - in_bytes);
    NJCHK(hipMemcpyAsync(back.data(), d + in_bytes, back.size(), hipMemcpyDeviceToHost, ctx->stream));
    if (ctx->sync(ctx->stream)) return PML_EDEVICE;
    if (ev_a) { float ms = 0; if (hipEventElapsedTime(&ms, ev_a, ev_b) == hipSuccess) ctx->pairsum_ms += ms; }
    for (int r = 0; r < nrep; ++r) {
        const size_t nn = reps[r].names.size() * reps[r].names.size();
        const long long *src = (const long long *)(back.data() + (o_out[r] - in_bytes));
        reps[r].sums.assign(src, src + nn);
    }
    return PML_OK;
}

// S = -1 + sum: the Java adds ints to a double that starts at -1 (Arrays.fill), exact below 2^53
void scores_of(const std::vector<long long> &sums, std::vector<double> &S) { S.resize(sums.size()); for (size_t i = 0; i < sums.size(); ++i) S[i] = (double)(sums[i] - 1); }

int tree_of(Ctx *ctx, const std::vector<std::string> &names, const std::vector<double> &S, int form, std::string &out) {
    std::string err;
    const int n = (int)names.size();
    const bool ok = form == PML_NJ_TREE ? nj_tree_string(n, names, S.data(), NJ_SIMILARITY, out, err) : nj_topology(n, names, S.data(), NJ_SIMILARITY, out, err);
    return ok ? PML_OK : ctx->fail(PML_EINVAL, err);
}

// The main NJ text with a support count behind the ')' of every inner node: the text is scanned once, a node's leaf set is
// looked up among the splits of the parsed tree (tips numbered in order of appearance, as Tree::parse_free numbers them).
std::string label_text(const std::string &text, const Tree &T, const std::vector<std::vector<int>> &counts) {
    const int n = T.ntax, words = (n + 63) / 64;
    auto canon = [&](std::vector<uint64_t> s) { if (s[0] & 1) for (int i = 0; i < n; ++i) s[i >> 6] ^= 1ULL << (i & 63); return s; };
    std::map<std::vector<uint64_t>, int> by_split;
    const auto L = leaf_sets(T);
    for (int v = n; v < T.nnodes(); ++v) for (int k = 0; k < 3; ++k) if (counts[v][k] >= 0) by_split[canon(L[(size_t)(v - n) * 3 + k])] = counts[v][k];
    std::string out; std::vector<std::vector<uint64_t>> stack; int tip = 0;
    for (size_t p = 0; p < text.size();) {
        const char c = text[p];
        if (c == '(') { stack.emplace_back((size_t)words, 0); out += c; ++p; }
        else if (c == ')') {
            std::vector<uint64_t> s = stack.back(); stack.pop_back();
            out += c; ++p;
            if (!stack.empty()) {
                for (int w = 0; w < words; ++w) stack.back()[w] |= s[w];
                auto it = by_split.find(canon(s));
                if (it != by_split.end()) out += std::to_string(it->second);
            }
        } else if (c == ':') { const size_t e = text.find_first_of(",()", p); out.append(text, p, e - p); p = e; }
        else if (c == ',' || c == ';') { out += c; ++p; }
        else {                                          // a leaf name
            const size_t e = text.find_first_of(",():;", p);
            if (!stack.empty() && tip < n) stack.back()[tip >> 6] |= 1ULL << (tip & 63);
            ++tip; out.append(text, p, e - p); p = e;
        }
    }
    return out;
}

std::vector<int> all_genes(int n) { std::vector<int> a((size_t)n); for (int i = 0; i < n; ++i) a[i] = i; return a; }
}  // namespace

extern "C" int pml_debug_pairscores(pml_ctx *ctx, const pml_alignment *aln, const int *table576, int chunk_sites, long long *out) {
    if (!ctx || !aln || !out || chunk_sites < 0) return PML_EINVAL;
    std::lock_guard<std::mutex> lk(ctx->c.mu);
    pml_fpguard fpg;
    pml_drop_worker_caches(ctx);
    try {
        PairScores ps; ps.ctx = &ctx->c;
        if (int rc = ps.run(1, aln, table576, chunk_sites)) return rc;
        std::vector<long long> m;
        if (int rc = ps.read(0, m)) return rc;
        std::copy(m.begin(), m.end(), out);
    } catch (const std::bad_alloc &) { return ctx->c.fail(PML_ENOMEM, "host allocation failed"); }
    catch (const std::exception &e) { return ctx->c.fail(PML_EINVAL, e.what()); }
    return PML_OK;
}

extern "C" int pml_pairwise_scores(pml_ctx *ctx, const pml_alignment *aln, const int *table576, double *scores_out) {
    if (!ctx || !aln || !scores_out) return PML_EINVAL;
    std::lock_guard<std::mutex> lk(ctx->c.mu);
    pml_fpguard fpg;
    pml_drop_worker_caches(ctx);
    try {
        PairScores ps; ps.ctx = &ctx->c;
        if (int rc = ps.run(1, aln, table576, 0)) return rc;
        std::vector<long long> m; std::vector<double> S;
        if (int rc = ps.read(0, m)) return rc;
        scores_of(m, S);
        std::copy(S.begin(), S.end(), scores_out);
    } catch (const std::bad_alloc &) { return ctx->c.fail(PML_ENOMEM, "host allocation failed"); }
    catch (const std::exception &e) { return ctx->c.fail(PML_EINVAL, e.what()); }
    return PML_OK;
}

extern "C" int pml_nj_tree(pml_ctx *ctx, const pml_alignment *aln, const int *table576, int form, char **newick_out) {
    if (newick_out) *newick_out = nullptr;
    if (!ctx || !aln || !newick_out) return PML_EINVAL;
    std::lock_guard<std::mutex> lk(ctx->c.mu);
    if (form != PML_NJ_TREE && form != PML_NJ_TOPOLOGY) return ctx->c.fail(PML_EINVAL, "form must be PML_NJ_TREE or PML_NJ_TOPOLOGY");
    if (aln->ntax < 4) return ctx->c.fail(PML_EINVAL, "neighbor joining needs at least 4 taxa (the reference returns null for 3)");
    pml_fpguard fpg;
    pml_drop_worker_caches(ctx);
    try {
        PairScores ps; ps.ctx = &ctx->c;
        if (int rc = ps.run(1, aln, table576, 0)) return rc;
        std::vector<long long> m; std::vector<double> S; std::string out;
        if (int rc = ps.read(0, m)) return rc;
        scores_of(m, S);
        std::vector<std::string> names(aln->names, aln->names + aln->ntax);
        if (int rc = tree_of(&ctx->c, names, S, form, out)) return rc;
        *newick_out = dup_cstr(out);
    } catch (const std::bad_alloc &) { return ctx->c.fail(PML_ENOMEM, "host allocation failed"); }
    catch (const std::exception &e) { return ctx->c.fail(PML_EINVAL, e.what()); }
    return *newick_out ? PML_OK : ctx->c.fail(PML_ENOMEM, "host allocation failed");
}

extern "C" int pml_nj_replicates(pml_ctx *ctx, int ngenes, const pml_alignment *genes, int nrep, int k, const int *sel, const int *table576,
                                 int form, char **newicks_out, double **scores_out, int **ntax_out) {
    if (newicks_out) *newicks_out = nullptr;
    if (scores_out) *scores_out = nullptr;
    if (ntax_out) *ntax_out = nullptr;
    if (!ctx || !genes || ngenes <= 0 || nrep <= 0 || !newicks_out) return PML_EINVAL;
    std::lock_guard<std::mutex> lk(ctx->c.mu);
    if (form != PML_NJ_TREE && form != PML_NJ_TOPOLOGY) return ctx->c.fail(PML_EINVAL, "form must be PML_NJ_TREE or PML_NJ_TOPOLOGY");
    if (!sel && nrep != 1) return ctx->c.fail(PML_EINVAL, "sel may be NULL only with nrep = 1 (all genes)");
    if (sel && k <= 0) return ctx->c.fail(PML_EINVAL, "k must be positive");
    pml_fpguard fpg;
    pml_drop_worker_caches(ctx);
    double *sc = nullptr; int *nt = nullptr;
    try {
        std::vector<std::vector<int>> sels;
        if (!sel) sels.push_back(all_genes(ngenes));
        else for (int r = 0; r < nrep; ++r) sels.emplace_back(sel + (size_t)r * k, sel + (size_t)(r + 1) * k);
        std::vector<Replicate> reps;
        if (int rc = replicate_scores(&ctx->c, ngenes, genes, sels, table576, reps)) return rc;
        std::string txt; std::vector<double> S, all_scores;
        nt = (int *)std::malloc(sizeof(int) * (size_t)nrep);
        if (!nt) return ctx->c.fail(PML_ENOMEM, "host allocation failed");
        for (int r = 0; r < nrep; ++r) {
            scores_of(reps[r].sums, S);
            nt[r] = (int)reps[r].names.size();
            all_scores.insert(all_scores.end(), S.begin(), S.end());
            std::string out;
            if (nt[r] < 4) { std::free(nt); return ctx->c.fail(PML_EINVAL, "replicate " + std::to_string(r) + " has " + std::to_string(nt[r]) + " taxa: neighbor joining needs at least 4"); }
            if (int rc = tree_of(&ctx->c, reps[r].names, S, form, out)) { std::free(nt); return rc; }
            txt += out; txt += '\n';
        }
        if (scores_out) {
            sc = (double *)std::malloc(sizeof(double) * std::max<size_t>(all_scores.size(), 1));
            if (!sc) { std::free(nt); return ctx->c.fail(PML_ENOMEM, "host allocation failed"); }
            std::copy(all_scores.begin(), all_scores.end(), sc);
        }
        *newicks_out = dup_cstr(txt);
        if (!*newicks_out) { std::free(nt); std::free(sc); return ctx->c.fail(PML_ENOMEM, "host allocation failed"); }
        if (scores_out) *scores_out = sc;
        if (ntax_out) *ntax_out = nt; else std::free(nt);
    } catch (const std::bad_alloc &) { std::free(nt); std::free(sc); return ctx->c.fail(PML_ENOMEM, "host allocation failed"); }
    catch (const std::exception &e) { std::free(nt); std::free(sc); return ctx->c.fail(PML_EINVAL, e.what()); }
    return PML_OK;
}

extern "C" int pml_nj_jackknife(pml_ctx *ctx, int ngenes, const pml_alignment *genes, const pml_jackknife_opts *opts, const int *table576,
                                int support_rule, char **main_newick_out, char **support_newicks_out) {
    if (main_newick_out) *main_newick_out = nullptr;
    if (support_newicks_out) *support_newicks_out = nullptr;
    if (!ctx || !genes || ngenes <= 0 || !main_newick_out) return PML_EINVAL;
    std::lock_guard<std::mutex> lk(ctx->c.mu);
    if (support_rule != PML_SUPPORT_EQUAL_TAXA && support_rule != PML_SUPPORT_DECORATOR && support_rule != PML_SUPPORT_RESTRICTED)
        return ctx->c.fail(PML_EINVAL, "bad support_rule " + std::to_string(support_rule));
    if (opts && opts->shard_world > 1) return ctx->c.fail(PML_EINVAL, "pml_nj_jackknife is not sharded: the whole loop is cheaper than a gather of its trees");
    const int reps = opts ? opts->reps : 100;
    if (reps < 0) return ctx->c.fail(PML_EINVAL, "reps must not be negative");
    pml_fpguard fpg;
    pml_drop_worker_caches(ctx);
    try {
        int subset = (opts && opts->subset_size > 0) ? opts->subset_size : ngenes / 2;
        subset = std::max(1, std::min(subset, ngenes));
        std::vector<int> draw((size_t)reps * subset + 1);
        if (reps > 0 && pml_jackknife_draw(ngenes, reps, subset, opts ? opts->seed : 0, draw.data()) != subset) return ctx->c.fail(PML_EINVAL, "the replicate draw failed");
        std::vector<std::vector<int>> sels{all_genes(ngenes)};
        for (int r = 0; r < reps; ++r) sels.emplace_back(draw.begin() + (size_t)r * subset, draw.begin() + (size_t)(r + 1) * subset);
        std::vector<Replicate> R;
        if (int rc = replicate_scores(&ctx->c, ngenes, genes, sels, table576, R)) return rc;
        std::vector<std::string> trees((size_t)reps + 1); std::vector<double> S;
        for (int r = 0; r <= reps; ++r) {
            if ((int)R[r].names.size() < 4) return ctx->c.fail(PML_EINVAL, (r ? "replicate " + std::to_string(r - 1) : std::string("the full alignment")) + " has fewer than 4 taxa");
            scores_of(R[r].sums, S);
            if (int rc = tree_of(&ctx->c, R[r].names, S, PML_NJ_TREE, trees[r])) return rc;
        }
        // supports: counted on the strings as returned, as pml_jackknife2 counts them
        Tree main; std::vector<std::string> names; std::string err, sup_txt;
        if (!Tree::parse_free(trees[0].c_str(), names, main, err)) return ctx->c.fail(PML_EPARSE, "main tree: " + err);
        std::vector<const char *> ptrs;
        for (int r = 1; r <= reps; ++r) { ptrs.push_back(trees[r].c_str()); sup_txt += trees[r]; sup_txt += '\n'; }
        std::vector<std::vector<int>> counts;
        if (!support_counts_rule(main, names, ptrs, support_rule, counts, err)) return ctx->c.fail(PML_EPARSE, err);
        *main_newick_out = dup_cstr(label_text(trees[0], main, counts));
        if (support_newicks_out) *support_newicks_out = dup_cstr(sup_txt);
        if (!*main_newick_out || (support_newicks_out && !*support_newicks_out)) {
            std::free(*main_newick_out); *main_newick_out = nullptr;
            if (support_newicks_out) { std::free(*support_newicks_out); *support_newicks_out = nullptr; }
            return ctx->c.fail(PML_ENOMEM, "host allocation failed");
        }
    } catch (const std::bad_alloc &) { return ctx->c.fail(PML_ENOMEM, "host allocation failed"); }
    catch (const std::exception &e) { return ctx->c.fail(PML_EINVAL, e.what()); }
    return PML_OK;
}

extern "C" int pml_pairscore_sum_stats(pml_ctx *ctx, long long *launches, double *total_ms) {
    if (!ctx) return PML_EINVAL;
    std::lock_guard<std::mutex> lk(ctx->c.mu);
    if (launches) *launches = ctx->c.pairsum_launches;
    if (total_ms) *total_ms = ctx->c.pairsum_ms;
    return PML_OK;
}
