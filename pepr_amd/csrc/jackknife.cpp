// jackknife.cpp -- gene-wise jackknife driver: the reference's data-parallel loop
// (PhylogenomicPipeline2.java:994-1126, 1227-1275, 1587-1633) as one native call.
// Concatenation follows MSAConcatenator.concatenate (MSAConcatenator.java:78-189): taxa = sorted
// union of the genes' taxon names, a gene that lacks a taxon contributes '?' columns.
// Gene alignments are encoded once into HBM; the full alignment and every replicate are gathered from them on
// the device (GeneStore / Batch::create_replicates) and the replicates are searched as ONE batch; the support counting is TreeSupportDecorator.addSupportValues (:86-163).
// pml_jackknife2 is the same loop under any model code (a model per replicate, its frequencies counted on the device by
// k_codehist), with another model for the support trees and the counting rules of host.hpp support_counts_rule.
// pml_jackknife3 adds PEPR's tree-building methods (-full_tree_method / -support_tree_method parsimony, parsimony_bl): parsimony
// trees of the resident genes, their Fitch tips written by k_fitch_tips (parsimony.hip) -- no CLV arena, no replicate code matrix.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <set>

#include "../../include/peprml.h"
#include "api_types.hpp"

using namespace pml;

namespace {
struct Concat { std::vector<std::string> names, rows; };

bool concatenate(int ngenes, const pml_alignment *genes, const std::vector<int> &sel, Concat &out, std::string &err) {
    std::set<std::string> uni;
    for (int g : sel) {
        if (g < 0 || g >= ngenes) { err = "gene index out of range"; return false; }
        const pml_alignment &A = genes[g];
        if (!A.names || !A.rows || A.ntax <= 0) { err = "bad alignment"; return false; }
        for (int i = 0; i < A.ntax; ++i) uni.insert(A.names[i]);
    }
    out.names.assign(uni.begin(), uni.end());           // std::set order == Arrays.sort for ASCII names
    out.rows.assign(out.names.size(), std::string());
    for (int g : sel) {
        const pml_alignment &A = genes[g];
        std::map<std::string, int> idx;
        for (int i = 0; i < A.ntax; ++i) idx[A.names[i]] = i;
        for (size_t t = 0; t < out.names.size(); ++t) {
            auto it = idx.find(out.names[t]);
            if (it == idx.end()) out.rows[t].append((size_t)A.nsites, '?');
            else {
                if ((int)strnlen(A.rows[it->second], (size_t)A.nsites) < A.nsites) { err = "row shorter than nsites"; return false; }
                out.rows[t].append(A.rows[it->second], (size_t)A.nsites);
            }
        }
    }
    return true;
}
// replicate r = `subset` genes drawn without replacement (partial Fisher-Yates on one mt19937_64 stream), sorted
std::vector<std::vector<int>> draw_subsets(int ngenes, int reps, int subset, unsigned long long seed) {
    std::mt19937_64 rng(seed);
    std::vector<std::vector<int>> rep((size_t)reps);
    std::vector<int> all(ngenes); for (int i = 0; i < ngenes; ++i) all[i] = i;
    for (int r = 0; r < reps; ++r) {
        std::vector<int> pool(all);
        for (int i = 0; i < subset; ++i) { const size_t j = i + (size_t)(rng() % (uint64_t)(ngenes - i)); std::swap(pool[i], pool[j]); }
        rep[r].assign(pool.begin(), pool.begin() + subset);
        std::sort(rep[r].begin(), rep[r].end());
    }
    return rep;
}
char *dup_cstr(const std::string &s) { char *p = (char *)std::malloc(s.size() + 1); if (p) std::memcpy(p, s.c_str(), s.size() + 1); return p; }
}  // namespace

extern "C" int pml_concatenate(int ngenes, const pml_alignment *genes, int nsel, const int *sel, char **fasta_out) {
    if (!genes || ngenes <= 0 || !fasta_out) return PML_EINVAL;
    *fasta_out = nullptr;
    try {
        std::vector<int> s;
        if (sel) s.assign(sel, sel + nsel); else { s.resize(ngenes); for (int i = 0; i < ngenes; ++i) s[i] = i; }
        Concat c; std::string err;
        if (!concatenate(ngenes, genes, s, c, err)) return PML_EINVAL;
        std::string txt;
        for (size_t i = 0; i < c.names.size(); ++i) { txt += '>'; txt += c.names[i]; txt += '\n'; txt += c.rows[i]; txt += '\n'; }
        *fasta_out = dup_cstr(txt);
    } catch (const std::exception &) { return PML_ENOMEM; }
    return *fasta_out ? PML_OK : PML_ENOMEM;
}

extern "C" int pml_jackknife_draw(int ngenes, int reps, int subset_size, unsigned long long seed, int *sel_out) {
    if (ngenes <= 0 || reps < 0 || !sel_out) return PML_EINVAL;
    int subset = subset_size > 0 ? subset_size : ngenes / 2;
    subset = std::max(1, std::min(subset, ngenes));
    try {
        const auto rep = draw_subsets(ngenes, reps, subset, seed);
        for (int r = 0; r < reps; ++r) std::copy(rep[r].begin(), rep[r].end(), sel_out + (size_t)r * subset);
    } catch (const std::exception &) { return PML_ENOMEM; }
    return subset;
}

// Test hook for SURVEY 8f-3: the code matrix + weights k_gather builds on the device for one gene selection, read back.
extern "C" int pml_debug_gather(pml_ctx *ctx, int ngenes, const pml_alignment *genes, int nsel, const int *sel,
                                int *ntax_out, int *npat_out, int *mpad_out, unsigned char **codes_out, double **weights_out,
                                char **names_out) {
    if (!ctx || !genes || ngenes <= 0 || !ntax_out || !npat_out || !mpad_out || !codes_out || !weights_out || !names_out) return PML_EINVAL;
    *codes_out = nullptr; *weights_out = nullptr; *names_out = nullptr;
    std::lock_guard<std::mutex> lk(ctx->c.mu);
    pml_drop_worker_caches(ctx);
    try {
        for (int g = 0; g < ngenes; ++g) if (!genes[g].names || !genes[g].rows || genes[g].ntax <= 0) return ctx->c.fail(PML_EINVAL, "bad alignment");
        std::vector<int> s;
        if (sel) s.assign(sel, sel + nsel); else { s.resize(ngenes); for (int i = 0; i < ngenes; ++i) s[i] = i; }
        GeneStore store;
        struct Drop { GeneStore &s; ~Drop() { s.destroy(); } } drop{store};
        if (int rc = store.create(&ctx->c, ngenes, reinterpret_cast<const pml_alignment_view *>(genes))) return rc;
        Batch b;
        struct DropB { Batch &b; ~DropB() { b.destroy(); } } dropb{b};
        if (int rc = b.create_replicates(&ctx->c, store, {s}, 0, 4, 1.0)) return rc;
        const Gene &G = b.genes[0];
        const size_t nt = (size_t)G.aln.ntax, mp = (size_t)G.aln.mpad;
        unsigned char *codes = (unsigned char *)std::malloc(nt * mp); double *w = (double *)std::malloc(mp * sizeof(double));
        if (!codes || !w) { std::free(codes); std::free(w); return ctx->c.fail(PML_ENOMEM, "host allocation failed"); }
        if (hipMemcpy(codes, G.d_codes, nt * mp, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(w, G.d_weight, mp * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) {
            std::free(codes); std::free(w); return ctx->c.fail(PML_EDEVICE, "read-back of the gathered matrix failed");
        }
        std::string names; for (auto &n : G.aln.names) { names += n; names += '\n'; }
        *ntax_out = (int)nt; *npat_out = G.aln.npat; *mpad_out = (int)mp; *codes_out = codes; *weights_out = w; *names_out = dup_cstr(names);
    } catch (const std::bad_alloc &) { return ctx->c.fail(PML_ENOMEM, "host allocation failed"); }
    catch (const std::exception &e) { return ctx->c.fail(PML_EINVAL, e.what()); }
    return PML_OK;
}

// the stepwise-addition seeds of pml_jackknife3's parsimony trees (peprml.h): idx 0 = the full tree, 1 + r = replicate r of the
// draw; 0 means "input order" to the core and is replaced
static unsigned parsimony_seed(unsigned long long seed, int idx) {
    const unsigned s = (unsigned)(seed + (unsigned long long)idx);
    return s ? s : 0x9E3779B9u;
}

// The loop itself, for pml_jackknife (one shared-model code, SUPPORT_EQUAL_TAXA), pml_jackknife2 (any valid code for the
// full tree and for the support trees, any counting rule) and pml_jackknife3 (a tree-building method for either kind of tree).
// The caller holds the context's mutex and has checked the codes and the methods.  mp_out (optional, 1 + reps): Fitch lengths.
static int jackknife_run(pml_ctx *ctx, int ngenes, const pml_alignment *genes, const pml_model *model, const pml_model *support_model,
                         int rule, const pml_jackknife_opts *opts, pml_result *main_out, char **support_out,
                         int full_method = PML_TREE_ML, int support_method = PML_TREE_ML, int pars_radius = 20, long long *mp_out = nullptr) {
    pml_fpguard fpg;
    std::memset(main_out, 0, sizeof *main_out);
    if (support_out) *support_out = nullptr;
    if (mp_out) for (int i = 0; i <= (opts ? std::max(opts->reps, 0) : 100); ++i) mp_out[i] = -1;
    const int reps = opts ? opts->reps : 100;
    int subset = (opts && opts->subset_size > 0) ? opts->subset_size : ngenes / 2;
    subset = std::max(1, std::min(subset, ngenes));
    const double eps = (opts && opts->epsilon > 0) ? opts->epsilon : 1e-3;
    const int spr_full = opts ? opts->spr_radius_full : 5;
    if (reps < 0) return PML_EINVAL;
    const int sworld = (opts && opts->shard_world > 1) ? opts->shard_world : 1, srank = sworld > 1 ? opts->shard_rank : 0;
    if (srank < 0 || srank >= sworld) return PML_EINVAL;
    pml_drop_worker_caches(ctx);
    try {
        std::vector<int> all(ngenes); for (int i = 0; i < ngenes; ++i) all[i] = i;
        for (int g = 0; g < ngenes; ++g) if (!genes[g].names || !genes[g].rows || genes[g].ntax <= 0) return ctx->c.fail(PML_EINVAL, "bad alignment");
        // every gene is encoded once and stays in HBM; the full alignment and each replicate are index lists over
        // that store, materialised by k_gather -- no concatenated text, no per-replicate encode
        GeneStore store;
        struct Drop { GeneStore &s; ~Drop() { s.destroy(); } } drop{store};
        static_assert(sizeof(pml_alignment) == sizeof(pml_alignment_view), "alignment view layout");
        if (int rc = store.create(&ctx->c, ngenes, reinterpret_cast<const pml_alignment_view *>(genes))) return rc;
        // replicates: seeded draw without replacement (reference: RandomSetUtils.getRandomSet, unseeded)
        std::vector<std::vector<int>> rep = draw_subsets(ngenes, reps, subset, opts ? opts->seed : 0);
        if (sworld > 1) {                       // this rank's replicates (all ranks drew the same lists)
            std::vector<std::vector<int>> mine;
            for (int r = srank; r < reps; r += sworld) mine.push_back(rep[r]);
            rep.swap(mine);
        }
        const int reps_here = (int)rep.size();
        const int ncat = model ? model->ncat : 4, pm = model ? model->pi_mode : 0;
        const double alpha = model ? model->alpha : 1.0;
        // the support trees' model (FastTree supports stay WAG while the full tree uses mlMatrix, PhylogenomicPipeline2.java:335-338)
        const int sncat = support_model ? support_model->ncat : 4, spm = support_model ? support_model->pi_mode : 0;
        const double salpha = support_model ? support_model->alpha : 1.0;
        const unsigned long long seed = opts ? opts->seed : 0;
        auto draw_index = [&](int r) { return srank + r * sworld; };          // this rank's replicate r in the draw's list
        if (support_method == PML_TREE_PARSIMONY) {          // refused before any tree is built, under the replicate's index in the draw
            for (int r = 0; r < reps_here; ++r) {
                std::set<std::string> taxa;
                for (int g : rep[r]) taxa.insert(store.items[g].aln.names.begin(), store.items[g].aln.names.end());
                if (taxa.size() < 3) return ctx->c.fail(PML_EPARSE, "replicate " + std::to_string(draw_index(r)) + ": parsimony needs at least 3 taxa");
            }
        }
        // full tree
        Tree main_tree; std::vector<std::string> main_names; double main_lnl = 0, main_alpha = full_method == PML_TREE_PARSIMONY ? 0.0 : alpha; int main_npat = 0, main_nsites = 0;
        if (srank == 0 && full_method != PML_TREE_ML) {
            // the parsimony tree of all genes, its tips written from the resident genes (k_fitch_tips)
            std::vector<Tree> pt; std::vector<std::vector<std::string>> pn; std::vector<long long> pl;
            if (int rc = parsimony_replicates(&ctx->c, store, {all}, {parsimony_seed(seed, 0)}, pars_radius, pt, pn, pl)) return rc;
            main_tree = pt[0]; main_names = pn[0];
            for (auto &it : store.items) { main_npat += it.aln.npat; main_nsites += it.aln.nsites; }
            if (mp_out) mp_out[0] = pl[0];
            if (full_method == PML_TREE_PARSIMONY_BL) {
                // `-f e -t` on that topology: lengths from 0.1 and alpha, as pml_optimize runs them
                Batch b;
                struct DropB { Batch &b; ~DropB() { b.destroy(); } } dropb{b};
                if (int rc = b.create_replicates(&ctx->c, store, {all}, pm, ncat, alpha)) return rc;
                Gene &G = b.genes[0];
                std::string err;
                if (G.aln.names != main_names || !Tree::parse(main_tree.newick(main_names, 6).c_str(), G.aln.names, G.tree, err))
                    return ctx->c.fail(PML_EINVAL, "parsimony tree does not fit the replicate of all genes: " + err);
                b.invalidate_all(0); G.mark_all(); ++b.topo_epoch;
                if (int rc = b.optimize(true, eps, &main_lnl)) return rc;
                main_tree = G.tree; main_alpha = G.alpha; main_npat = G.aln.npat; main_nsites = G.aln.nsites;
            }
        } else if (srank == 0) {
            Batch b; int rc = b.create_replicates(&ctx->c, store, {all}, pm, ncat, alpha);
            if (!rc) rc = b.search(true, spr_full, true, eps, &main_lnl);
            if (rc) { b.destroy(); return rc; }
            main_tree = b.genes[0].tree; main_names = b.genes[0].aln.names; main_alpha = b.genes[0].alpha; main_npat = b.genes[0].aln.npat; main_nsites = b.genes[0].aln.nsites;
            b.destroy();
        }
        // support trees: one device batch, or consecutive sub-batches when the replicates' CLV arenas do not fit in free
        // HBM together (a replicate of 100 taxa x 10^5 patterns needs ~19 GB in search mode)
        std::vector<Tree> sup((size_t)reps_here);
        std::string sup_txt;
        if (reps_here > 0) {
            size_t free_b = 0, total_b = 0;
            if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = (size_t)1 << 40;
            size_t budget = (size_t)(0.85 * (double)(free_b + ctx->c.arena_cache_bytes));
            if (const char *e = std::getenv("PML_HBM_BUDGET_MB")) budget = (size_t)std::atoll(e) << 20;   // test hook
            auto rep_bytes = [&](const std::vector<int> &sel) {
                size_t pats = 0; std::set<std::string> taxa;
                for (int g : sel) { pats += (size_t)store.items[g].aln.npat; taxa.insert(store.items[g].aln.names.begin(), store.items[g].aln.names.end()); }
                const size_t mp = (pats + 31) / 32 * 32, nt = std::max<size_t>(taxa.size(), 3), slots = 3 * (nt - 2) + NSCRATCH + MAXTAIL;
                return slots * CLV_ROWS * ((mp + 127) / 128 * 128) * 8 + slots * mp * 4 + nt * mp + 64 * mp + (1 << 16);
            };
            // a parsimony replicate holds its Fitch pool alone: tips, 3 messages per inner node and radius + 2 path vectors for
            // each of at most 64 prune groups, 4 B per pattern each -- no CLV arena
            auto pars_bytes = [&](const std::vector<int> &sel) {
                size_t pats = 0; std::set<std::string> taxa;
                for (int g : sel) { pats += (size_t)store.items[g].aln.npat; taxa.insert(store.items[g].aln.names.begin(), store.items[g].aln.names.end()); }
                const size_t mp = std::max<size_t>(32, (pats + 31) / 32 * 32), nt = std::max<size_t>(taxa.size(), 3), groups = pars_radius > 0 ? 64 : 1;
                return (nt + 3 * (nt - 2) + groups * (size_t)(pars_radius + 2)) * mp * 4 + mp * 4;
            };
            if (support_method == PML_TREE_PARSIMONY && ctx->c.arena_cache) {
                // the pools are allocations of their own: the full tree's arena goes back to the driver, as the budget counts it
                hipFree(ctx->c.arena_cache); ctx->c.arena_cache = nullptr; ctx->c.arena_cache_bytes = 0;
            }
            for (int begin = 0; begin < reps_here && support_method == PML_TREE_PARSIMONY;) {
                size_t used = 0; int end = begin;
                while (end < reps_here) { const size_t need = pars_bytes(rep[end]); if (end > begin && used + need > budget) break; used += need; ++end; }
                std::vector<std::vector<int>> part(rep.begin() + begin, rep.begin() + end);
                std::vector<unsigned> seeds;
                for (int r = begin; r < end; ++r) seeds.push_back(parsimony_seed(seed, 1 + draw_index(r)));
                std::vector<Tree> pt; std::vector<std::vector<std::string>> pn; std::vector<long long> pl;
                if (int rc = parsimony_replicates(&ctx->c, store, part, seeds, pars_radius, pt, pn, pl)) return rc;
                for (int r = begin; r < end; ++r) {
                    const std::string nw = pt[r - begin].newick(pn[r - begin], -1);       // topology only, as pml_parsimony prints
                    sup_txt += nw; sup_txt += '\n';
                    if (mp_out) mp_out[1 + draw_index(r)] = pl[r - begin];
                    if (srank != 0 || rule != SUPPORT_EQUAL_TAXA) continue;
                    if (pn[r - begin] == main_names) sup[r] = pt[r - begin];
                    else { std::string e2; Tree t; if (Tree::parse(nw.c_str(), main_names, t, e2)) sup[r] = t; else sup[r] = Tree(); }
                }
                begin = end;
            }
            for (int begin = 0; begin < reps_here && support_method == PML_TREE_ML;) {
                size_t used = 0; int end = begin;
                while (end < reps_here) { const size_t need = rep_bytes(rep[end]); if (end > begin && used + need > budget) break; used += need; ++end; }
                std::vector<std::vector<int>> part(rep.begin() + begin, rep.begin() + end);
                Batch b; int rc = b.create_replicates(&ctx->c, store, part, spm, sncat, salpha);
                std::vector<double> l(end - begin);
                if (!rc) rc = b.search(true, 0, true, eps, l.data());
                if (rc) { b.destroy(); return rc; }
                for (int r = begin; r < end; ++r) {
                    const Gene &G = b.genes[r - begin];
                    const std::string nw = G.tree.newick(G.aln.names, 6);
                    sup_txt += nw; sup_txt += '\n';
                    // a replicate may lack taxa that occur only in unselected genes: such trees cannot
                    // contain the main tree's bipartitions and are counted as not supporting
                    if (srank != 0 || rule != SUPPORT_EQUAL_TAXA) continue;
                    if (G.aln.names == main_names) sup[r] = G.tree;
                    else { std::string e2; Tree t; if (Tree::parse(nw.c_str(), main_names, t, e2)) sup[r] = t; else sup[r] = Tree(); }
                }
                b.destroy();
                begin = end;
            }
        }
        std::vector<Tree> usable;
        for (auto &t : sup) if (t.ntax == main_tree.ntax) usable.push_back(t);
        std::vector<std::vector<int>> counts;
        if (srank == 0 && rule == SUPPORT_EQUAL_TAXA) counts = support_counts(main_tree, usable);
        else if (srank == 0) {             // the other rules read the support trees as the caller will: the returned strings
            std::vector<std::string> lines; std::vector<const char *> ptrs; std::string err;
            for (size_t b = 0, e; b < sup_txt.size(); b = e + 1) { e = sup_txt.find('\n', b); lines.push_back(sup_txt.substr(b, e - b)); }
            for (auto &l : lines) ptrs.push_back(l.c_str());
            if (!support_counts_rule(main_tree, main_names, ptrs, rule, counts, err)) return ctx->c.fail(PML_EPARSE, err);
        }
        const bool topo_only = full_method == PML_TREE_PARSIMONY;          // a parsimony tree has no lengths: `)87`
        const std::string out = srank == 0 ? main_tree.newick_labeled(main_names, topo_only ? -1 : 6, counts) : std::string();
        main_out->lnl = main_lnl; main_out->alpha = main_alpha; main_out->tree_length = topo_only ? 0.0 : main_tree.length();
        main_out->npatterns = main_npat; main_out->nsites = main_nsites;
        if (srank == 0) main_out->newick = dup_cstr(out);
        if (support_out) *support_out = dup_cstr(sup_txt);
        if (srank == 0 && !main_out->newick) return ctx->c.fail(PML_ENOMEM, "host allocation failed");
    } catch (const std::bad_alloc &) { return ctx->c.fail(PML_ENOMEM, "host allocation failed"); }
    catch (const std::exception &e) { return ctx->c.fail(PML_EINVAL, e.what()); }
    return PML_OK;
}

extern "C" int pml_jackknife(pml_ctx *ctx, int ngenes, const pml_alignment *genes, const pml_model *model,
                             const pml_jackknife_opts *opts, pml_result *main_out, char **support_out) {
    if (!ctx || !genes || ngenes <= 0 || !main_out) return PML_EINVAL;
    std::memset(main_out, 0, sizeof *main_out);
    if (support_out) *support_out = nullptr;
    std::lock_guard<std::mutex> lk(ctx->c.mu);
    // this entry keeps one shared model for the full tree and the replicates: the per-gene codes are refused here, before
    // anything is encoded or uploaded (pml_jackknife2 builds a model per replicate)
    if (model && !ctx->c.valid_code(model->pi_mode)) return ctx->c.fail(PML_EINVAL, "bad pi_mode " + std::to_string(model->pi_mode));
    if (model && model_per_gene(model->pi_mode))
        return ctx->c.fail(PML_EINVAL, ctx->c.model_name(model->pi_mode) + " is not available for the gene-wise jackknife: its replicates are gathered on the device and "
                                       "carry one shared model (use PROTGAMMAWAG or a registered matrix with its own frequencies)");
    return jackknife_run(ctx, ngenes, genes, model, model, SUPPORT_EQUAL_TAXA, opts, main_out, support_out);
}

extern "C" int pml_jackknife2(pml_ctx *ctx, int ngenes, const pml_alignment *genes, const pml_model *full_model,
                              const pml_jackknife_opts2 *opts, pml_result *main_out, char **support_out) {
    if (!ctx || !genes || ngenes <= 0 || !main_out) return PML_EINVAL;
    std::memset(main_out, 0, sizeof *main_out);
    if (support_out) *support_out = nullptr;
    const int rule = opts ? opts->support_rule : PML_SUPPORT_EQUAL_TAXA;
    const pml_model *sm = (opts && opts->support_model) ? opts->support_model : full_model;
    std::lock_guard<std::mutex> lk(ctx->c.mu);
    if (rule != PML_SUPPORT_EQUAL_TAXA && rule != PML_SUPPORT_DECORATOR && rule != PML_SUPPORT_RESTRICTED) return ctx->c.fail(PML_EINVAL, "bad support_rule " + std::to_string(rule));
    for (const pml_model *m : {full_model, sm}) {
        if (m && !ctx->c.valid_code(m->pi_mode)) return ctx->c.fail(PML_EINVAL, "bad pi_mode " + std::to_string(m->pi_mode));
        if (m && m->ncat != 1 && m->ncat != 4) return ctx->c.fail(PML_EINVAL, "ncat must be 1 or 4");
    }
    return jackknife_run(ctx, ngenes, genes, full_model, sm, rule, opts ? &opts->base : nullptr, main_out, support_out);
}

extern "C" int pml_jackknife3(pml_ctx *ctx, int ngenes, const pml_alignment *genes, const pml_model *full_model,
                              const pml_jackknife_opts3 *opts, pml_result *main_out, char **support_out, long long *mp_lengths_out) {
    if (!ctx || !genes || ngenes <= 0 || !main_out) return PML_EINVAL;
    std::memset(main_out, 0, sizeof *main_out);
    if (support_out) *support_out = nullptr;
    const pml_jackknife_opts2 *o2 = opts ? &opts->base2 : nullptr;
    const int rule = o2 ? o2->support_rule : PML_SUPPORT_EQUAL_TAXA;
    const int fm = opts ? opts->full_method : PML_TREE_ML, sm_ = opts ? opts->support_method : PML_TREE_ML, radius = opts ? opts->parsimony_radius : 20;
    const pml_model *sm = (o2 && o2->support_model) ? o2->support_model : full_model;
    std::lock_guard<std::mutex> lk(ctx->c.mu);
    // everything is refused here, before a gene is encoded or uploaded
    if (rule != PML_SUPPORT_EQUAL_TAXA && rule != PML_SUPPORT_DECORATOR && rule != PML_SUPPORT_RESTRICTED) return ctx->c.fail(PML_EINVAL, "bad support_rule " + std::to_string(rule));
    if (fm != PML_TREE_ML && fm != PML_TREE_PARSIMONY && fm != PML_TREE_PARSIMONY_BL) return ctx->c.fail(PML_EINVAL, "bad full_method " + std::to_string(fm));
    if (sm_ == PML_TREE_PARSIMONY_BL)
        return ctx->c.fail(PML_EINVAL, "support_method PML_TREE_PARSIMONY_BL is not built: nothing reads a support tree's branch lengths (use PML_TREE_PARSIMONY)");
    if (sm_ != PML_TREE_ML && sm_ != PML_TREE_PARSIMONY) return ctx->c.fail(PML_EINVAL, "bad support_method " + std::to_string(sm_));
    if (radius < 0) return ctx->c.fail(PML_EINVAL, "parsimony_radius must not be negative");
    // a model is checked where a tree is built under it
    const pml_model *used[2] = {fm == PML_TREE_PARSIMONY ? nullptr : full_model, sm_ == PML_TREE_PARSIMONY ? nullptr : sm};
    for (const pml_model *m : used) {
        if (m && !ctx->c.valid_code(m->pi_mode)) return ctx->c.fail(PML_EINVAL, "bad pi_mode " + std::to_string(m->pi_mode));
        if (m && m->ncat != 1 && m->ncat != 4) return ctx->c.fail(PML_EINVAL, "ncat must be 1 or 4");
    }
    return jackknife_run(ctx, ngenes, genes, full_model, sm, rule, o2 ? &o2->base : nullptr, main_out, support_out, fm, sm_, radius, mp_lengths_out);
}

// Test hook for k_fitch_tips, as pml_debug_gather is for k_gather: the Fitch tip rows and weights of one gene selection, read back.
extern "C" int pml_debug_fitch_tips(pml_ctx *ctx, int ngenes, const pml_alignment *genes, int nsel, const int *sel, int *ntax_out,
                                    int *npat_out, int *mpad_out, unsigned **masks_out, int **weights_out, char **names_out) {
    if (!ctx || !genes || ngenes <= 0 || !ntax_out || !npat_out || !mpad_out || !masks_out || !weights_out || !names_out || (sel && nsel <= 0)) return PML_EINVAL;
    *masks_out = nullptr; *weights_out = nullptr; *names_out = nullptr;
    std::lock_guard<std::mutex> lk(ctx->c.mu);
    pml_drop_worker_caches(ctx);
    try {
        for (int g = 0; g < ngenes; ++g) if (!genes[g].names || !genes[g].rows || genes[g].ntax <= 0) return ctx->c.fail(PML_EINVAL, "bad alignment");
        std::vector<int> s;
        if (sel) s.assign(sel, sel + nsel); else { s.resize(ngenes); for (int i = 0; i < ngenes; ++i) s[i] = i; }
        GeneStore store;
        struct Drop { GeneStore &s; ~Drop() { s.destroy(); } } drop{store};
        if (int rc = store.create(&ctx->c, ngenes, reinterpret_cast<const pml_alignment_view *>(genes))) return rc;
        std::vector<unsigned> masks; std::vector<int> w; std::vector<std::string> nm;
        if (int rc = fitch_tips_readback(&ctx->c, store, s, npat_out, mpad_out, masks, w, nm)) return rc;
        unsigned *pm = (unsigned *)std::malloc(masks.size() * sizeof(unsigned)); int *pw = (int *)std::malloc(w.size() * sizeof(int));
        if (!pm || !pw) { std::free(pm); std::free(pw); return ctx->c.fail(PML_ENOMEM, "host allocation failed"); }
        std::memcpy(pm, masks.data(), masks.size() * sizeof(unsigned)); std::memcpy(pw, w.data(), w.size() * sizeof(int));
        std::string names; for (auto &n : nm) { names += n; names += '\n'; }
        *ntax_out = (int)nm.size(); *masks_out = pm; *weights_out = pw; *names_out = dup_cstr(names);
    } catch (const std::bad_alloc &) { return ctx->c.fail(PML_ENOMEM, "host allocation failed"); }
    catch (const std::exception &e) { return ctx->c.fail(PML_EINVAL, e.what()); }
    return PML_OK;
}

// Test hook for k_codehist: the selection is gathered TOGETHER with the replicate of all genes (one batch, one k_codehist
// launch over two replicates that may differ in taxa and patterns) and its histogram and frequencies are read back.
extern "C" int pml_debug_replicate_freqs(pml_ctx *ctx, int ngenes, const pml_alignment *genes, int nsel, const int *sel,
                                         long long counts_out[23], double pi_out[20]) {
    if (!ctx || !genes || ngenes <= 0 || !counts_out || !pi_out || (sel && nsel <= 0)) return PML_EINVAL;
    pml_fpguard fpg;
    std::lock_guard<std::mutex> lk(ctx->c.mu);
    pml_drop_worker_caches(ctx);
    try {
        for (int g = 0; g < ngenes; ++g) if (!genes[g].names || !genes[g].rows || genes[g].ntax <= 0) return ctx->c.fail(PML_EINVAL, "bad alignment");
        std::vector<int> all(ngenes); for (int i = 0; i < ngenes; ++i) all[i] = i;
        std::vector<std::vector<int>> reps{all};
        if (sel) reps.emplace_back(sel, sel + nsel);
        GeneStore store;
        struct Drop { GeneStore &s; ~Drop() { s.destroy(); } } drop{store};
        if (int rc = store.create(&ctx->c, ngenes, reinterpret_cast<const pml_alignment_view *>(genes))) return rc;
        Batch b;
        struct DropB { Batch &b; ~DropB() { b.destroy(); } } dropb{b};
        if (int rc = b.create_replicates(&ctx->c, store, reps, PML_PI_EMPIRICAL, 4, 1.0)) return rc;
        const Gene &G = b.genes.back();
        std::copy(G.code_hist.begin(), G.code_hist.end(), counts_out);
        std::copy(G.counted_pi.begin(), G.counted_pi.end(), pi_out);
    } catch (const std::bad_alloc &) { return ctx->c.fail(PML_ENOMEM, "host allocation failed"); }
    catch (const std::exception &e) { return ctx->c.fail(PML_EINVAL, e.what()); }
    return PML_OK;
}

// Non-parametric bootstrap (`raxmlHPC -f a -x seed -N reps`, RAxMLRunner.java:115-132 with reps > 0): best ML tree
// of the alignment (NNI + lazy SPR) and `reps` trees of column-resampled alignments (NNI), searched as ONE device
// batch; the best tree carries the percentage of replicates containing each bipartition (RAxML_bipartitions.<n>).
// RAxML's "rapid" heuristics (CAT approximation, tree reuse between replicates) are not restated: each replicate
// gets a full search, which is what those heuristics approximate.
extern "C" int pml_bootstrap(pml_ctx *ctx, const pml_alignment *aln, const pml_model *model, int reps, unsigned long long seed,
                             int spr_radius_best, double epsilon, pml_result *best_out, char **replicate_newicks_out) {
    if (!ctx || !aln || !best_out || reps < 0 || aln->ntax < 3 || aln->nsites < 1) return PML_EINVAL;
    pml_fpguard fpg;
    std::memset(best_out, 0, sizeof *best_out);
    if (replicate_newicks_out) *replicate_newicks_out = nullptr;
    const double eps = epsilon > 0 ? epsilon : 1e-3;
    std::lock_guard<std::mutex> lk(ctx->c.mu);
    pml_drop_worker_caches(ctx);
    try {
        const int ncat = model ? model->ncat : 4, pm = model ? model->pi_mode : 0;
        const double alpha = model ? model->alpha : 1.0;
        const int n = aln->ntax, L = aln->nsites;
        Tree best; std::vector<std::string> names; double lnl = 0, al = alpha; int npat = 0;
        {
            pml_alignment_view v{n, L, aln->names, aln->rows};
            Batch b; int rc = b.create(&ctx->c, 1, &v, nullptr, pm, ncat, alpha, false);
            if (!rc) rc = b.search(true, spr_radius_best, true, eps, &lnl);
            if (rc) { b.destroy(); return rc; }
            best = b.genes[0].tree; names = b.genes[0].aln.names; al = b.genes[0].alpha; npat = b.genes[0].aln.npat;
            b.destroy();
        }
        std::vector<Tree> trees((size_t)reps); std::string txt;
        if (reps > 0) {
            std::mt19937_64 rng(seed);
            std::vector<std::vector<std::string>> rows((size_t)reps, std::vector<std::string>((size_t)n, std::string((size_t)L, '-')));
            std::vector<int> col((size_t)L);
            for (int r = 0; r < reps; ++r) {
                for (int s = 0; s < L; ++s) col[s] = (int)(rng() % (uint64_t)L);
                for (int i = 0; i < n; ++i) { const char *src = aln->rows[i]; std::string &dst = rows[r][i]; for (int s = 0; s < L; ++s) dst[s] = src[col[s]]; }
            }
            std::vector<std::vector<const char *>> rps((size_t)reps);
            std::vector<pml_alignment_view> vs((size_t)reps);
            for (int r = 0; r < reps; ++r) { for (auto &x : rows[r]) rps[r].push_back(x.c_str()); vs[r] = pml_alignment_view{n, L, aln->names, rps[r].data()}; }
            // one device batch, or consecutive sub-batches when the replicates do not fit in free HBM together
            size_t free_b = 0, total_b = 0;
            if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = (size_t)1 << 40;
            size_t budget = (size_t)(0.85 * (double)(free_b + ctx->c.arena_cache_bytes));
            if (const char *e = std::getenv("PML_HBM_BUDGET_MB")) budget = (size_t)std::atoll(e) << 20;   // test hook
            const size_t mp = ((size_t)L + 31) / 32 * 32, slots = 3 * ((size_t)n - 2) + NSCRATCH + MAXTAIL;
            const size_t per_rep = slots * CLV_ROWS * ((mp + 127) / 128 * 128) * 8 + slots * mp * 4 + (size_t)n * mp + 64 * mp + (1 << 16);
            const int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)reps, budget / per_rep));
            for (int begin = 0; begin < reps; begin += chunk) {
                const int m = std::min(chunk, reps - begin);
                Batch b; int rc = b.create(&ctx->c, m, vs.data() + begin, nullptr, pm, ncat, alpha, false);
                std::vector<double> l((size_t)m);
                if (!rc) rc = b.search(true, 0, true, eps, l.data());
                if (rc) { b.destroy(); return rc; }
                for (int r = 0; r < m; ++r) { trees[begin + r] = b.genes[r].tree; txt += b.genes[r].tree.newick(names, 6); txt += '\n'; }
                b.destroy();
            }
        }
        auto counts = support_counts(best, trees);
        if (reps > 0) for (auto &row : counts) for (int &c : row) if (c >= 0) c = (int)(0.5 + 100.0 * c / reps);   // percent, as RAxML_bipartitions
        best_out->lnl = lnl; best_out->alpha = al; best_out->tree_length = best.length(); best_out->npatterns = npat; best_out->nsites = L;
        best_out->newick = dup_cstr(reps > 0 ? best.newick_labeled(names, 6, counts) : best.newick(names, 6));
        if (replicate_newicks_out) *replicate_newicks_out = dup_cstr(txt);
        if (!best_out->newick) return ctx->c.fail(PML_ENOMEM, "host allocation failed");
    } catch (const std::bad_alloc &) { return ctx->c.fail(PML_ENOMEM, "host allocation failed"); }
    catch (const std::exception &e) { return ctx->c.fail(PML_EINVAL, e.what()); }
    return PML_OK;
}
