// engine.hpp -- device-resident gene batches and the host-side schedulers that drive the kernels.
#pragma once
#include <hip/hip_runtime.h>

#include <array>
#include <mutex>
#include <string>
#include <vector>

#include "host.hpp"
#include "kernels.h"

namespace pml {

constexpr int MAXTAIL = 4;            // tail requests (evaluate / sumtable+Newton) per gene per run()

enum { K_PMAT = 0, K_NEWVIEW = 1, K_EVALUATE = 2, K_SUMTABLE = 3, K_NEWTON = 4, K_REDUCE = 5, K_HOST_BUILD = 6, K_HOST_WAIT = 7, K_MODEL = 8, K_CODEHIST = 9, K_PAIRSCORE = 10, K_COLSPLIT = 11, K_SPLITCOST = 12, K_TREEPAIRS = 13, K_COUNT = 14 };

// Model codes (pml_model.pi_mode): 0 / 1 WAG with fixed frequencies, 2 WAG with the gene's empirical frequencies, 3 GTR
// (exchangeabilities estimated per gene, empirical frequencies), 16 + 2 i the i-th registered matrix with its own
// frequencies, 17 + 2 i its exchangeabilities with empirical frequencies.  A code is either SHARED (one eigen-system per
// context, cached) or PER GENE (every gene of a batch carries its own ModelDev): the one predicate that decides.
enum { PM_GTR = 3, PM_REGISTERED = 16 };
inline bool model_per_gene(int pm) { return pm == 2 || pm == PM_GTR || (pm >= PM_REGISTERED && (pm & 1)); }
constexpr double RATE_MIN = 1e-7, RATE_MAX = 1e6;     // bounds of an estimated exchangeability (the last of the 190 is fixed at 1)
struct Matrix { std::string name; double exch[NEXCH]; double pi[NS]; };

struct Ctx {
    int device = 0;
    bool profile = false;
    hipStream_t stream = nullptr;
    std::mutex mu;
    std::string last_error;
    // one eigen-system per SHARED model code used on this context so far: the model and its 2*PFRAG eigen-basis fragments
    struct Shared { int code; ModelDev *d_model; double *d_eigfrags; };
    std::vector<Shared> shared;
    const Shared *shared_of(int pm) const { for (auto &m : shared) if (m.code == pm) return &m; return nullptr; }
    // registered rate matrices (pml_matrix_register) live on the context the caller created; its worker contexts read them
    // through `root` (registration and every batch creation hold the root's mutex)
    const Ctx *root = nullptr;
    std::vector<Matrix> matrices;
    const Matrix *matrix_of(int pm) const;        // null: not a registered code
    bool valid_code(int pm) const { return (pm >= 0 && pm <= PM_GTR) || matrix_of(pm) != nullptr; }
    std::string model_name(int pm) const;         // the RAxML name of a code, for messages
    struct KStat { long long launches = 0; double ms = 0; double bytes = 0; double flops = 0; } stats[K_COUNT];
    long long pairsum_launches = 0; double pairsum_ms = 0;      // k_pairscore_sum launches and (profile mode) their HIP-event time (pml_pairscore_sum_stats)
    long long newton_giveups = 0, newton_reissued = 0, newton_seq_launches = 0;   // k_newton fallback statistics (pml_newton_fallbacks)
    long long fitch_tips_launches = 0, fitch_launches = 0;      // k_fitch_tips and k_fitch launches (pml_fitch_stats)
    long long colclass_launches = 0, colgather_launches = 0; double trim_ms[3] = {0, 0, 0};   // pml_trim_stats: k_colclass, k_colgather, the uploads
    long long gbclass_launches = 0, gbselect_launches = 0; double gb_ms[3] = {0, 0, 0};       // pml_gblocks_stats: k_gbclass, k_gbselect, the uploads
    long long gs_launches[5] = {0, 0, 0, 0, 0}; double gs_ms[5] = {0, 0, 0, 0, 0};   // pml_gene_steps_stats: k_fitch_sitesteps, k_steps_expand, k_colminsteps, k_steps_resample, k_steps_table
    // pml_boot_stats: k_boot_count, k_boot_index, k_boot_gather, k_boot_pairs launches, (profile mode) their HIP-event times, and the
    // host wall time of the replicate builds (count .. NJ starts / tip rows)
    long long boot_launches[4] = {0, 0, 0, 0}; double boot_ms[4] = {0, 0, 0, 0}, boot_build_ms = 0;
    // pml_mash_stats: k_mash_hash, k_mash_cut, k_mash_compact, k_mash_unique, k_mash_pairs launches; (profile mode) HIP-event times of
    // the uploads, k_mash_hash, the selection (cut .. unique) and k_mash_pairs; sub-batches whose cut was raised and repeated
    long long mash_launches[5] = {0, 0, 0, 0, 0}, mash_repeats = 0; double mash_ms[4] = {0, 0, 0, 0};
    bool mash_full_sort = false;                                 // pml_debug_mash_full_sort: every genome's cut takes everything
    // pml_mcl_stats: k_mcl_fill, k_mcl_lds<packed>, k_mcl_lds, k_mcl_expand, k_mcl_inflate, k_mcl_flag, k_mcl_read launches and sub-batches;
    // (profile mode) HIP-event times of uploads and fill, the packed class, the LDS class, the HBM class
    long long mcl_launches[8] = {0, 0, 0, 0, 0, 0, 0, 0}; double mcl_ms[4] = {0, 0, 0, 0};
    // pml_sw_stats: k_sw_score launches per class and work units, the DP cells they covered; (profile mode) HIP-event times of the classes and the uploads
    long long sw_launches[4] = {0, 0, 0, 0}, sw_cells = 0; double sw_ms[4] = {0, 0, 0, 0};
    // pml_msa_stats: k_msa_colv, k_msa_dp, k_msa_walk, k_msa_gather launches (k_msa_counts, one a call, with the first), merges, levels,
    // sub-batches, DP cells; (profile mode) HIP-event times of the four
    long long msa_counts[8] = {0, 0, 0, 0, 0, 0, 0, 0}; double msa_ms[4] = {0, 0, 0, 0};
    std::vector<double> boot_last_lnl;                          // the ML replicates' lnL of the last pml_bootstrap2 call (pml_boot_replicate_lnls)
    struct Ev { int kind; hipEvent_t a, b; };
    std::vector<Ev> pending;
    std::vector<hipEvent_t> pool;
    // the last destroyed batch's device arena, kept for the next batch: the driver zero-fills fresh allocations at
    // ~40 GB/s (a 111 GiB C4 arena costs 3-6 s), so back-to-back batches (full tree then replicates, successive
    // one-shot calls) reuse it; released by destroy() or when a larger one replaces it
    char *arena_cache = nullptr; size_t arena_cache_bytes = 0;

    int init(int dev, bool prof);
    // a worker context of a grouped search call (api.cpp): its own stream (highest priority class: its own pool of hardware
    // queues), events, statistics and arena cache
    int init_worker(const Ctx &parent);
    bool owns_stream = true;
    hipEvent_t ev_sync = nullptr;
    int sync(hipStream_t s);             // wait for everything THIS context has enqueued on s so far (event-based: other users of a shared stream may enqueue behind it)
    void destroy();
    int ensure_model(int pi_mode);
    hipEvent_t get_event();
    void tic(int kind, double bytes, double flops = 0);   // record start (profile mode); bytes / flops = SURVEY 8d per-operation figures
    void toc();                          // record stop
    // tic + toc for ONE launch that records its own start and end (launch_* start / stop): the pair of events to hand to it
    // (null when not profiling).  No marker packets between the kernels of a step
    Ev tic_self(int kind, double bytes, double flops = 0);
    void resolve_events();               // after a stream sync
    int fail(int code, const std::string &msg) { last_error = msg; return code; }
};

struct Gene {
    EncodedAlignment aln;
    Tree tree;
    double alpha = 1.0;
    double rates[NCAT] = {1, 1, 1, 1};
    unsigned rates_epoch = 0;      // bumped by set_alpha (cached score plans refresh a gene's rates only when it moved)
    int model_code = 0;            // pml_model.pi_mode of this gene (pml_model_eval: one batch, a code per gene)
    // device-gathered replicates under a per-gene code: the weighted histogram of the 23 codes (k_codehist) and the empirical
    // frequencies it gives; empty for genes encoded from text, whose frequencies are counted by empirical_freqs
    std::vector<long long> code_hist; std::vector<double> counted_pi;
    // device pointers (inside the batch arena)
    uint8_t *d_codes = nullptr;
    double *d_weight = nullptr;
    double *d_clv = nullptr;       // slot_cap slots of 80*mpad doubles
    int *d_scl = nullptr;          // slot_cap slots of mpad ints
    double *d_sumtab[MAXTAIL] = {};    // 80*mpad each
    int *d_sumscl[MAXTAIL] = {};       // mpad each
    double *d_patlnl[MAXTAIL] = {};    // mpad each
    int slot_cap = 0, next_slot = 0;
    int nscratch = 0;              // scratch CLV slots behind the slot_cap message slots (NSCRATCH; more in a search2 batch)
    std::vector<int> slot_of;      // directed-edge index (v-ntax)*3+k -> slot (-1 = none)
    std::vector<uint8_t> valid;
    std::vector<int> pend_level;   // scratch for collection (-1 = not pending)
    std::vector<Constraint> cons;  // topological constraints of the running search (empty = none)
    std::vector<uint8_t> dirty;    // [node*3+slot]: branch needs re-optimisation (both directions set)
    double *d_len = nullptr;       // [node*3+slot] device copies of branch lengths written by k_newton (chained passes)
    std::vector<uint8_t> len_pending;   // [node*3+slot]: the current length lives in d_len, the host value is stale
    void mark_node(int v) { for (int k = 0; k < 3; ++k) { const int w = tree.nbr[v][k]; if (w < 0) continue; dirty[v * 3 + k] = 1; dirty[w * 3 + tree.slot(w, v)] = 1; } }
    void mark_all() { dirty.assign((size_t)tree.nnodes() * 3, 1); }
    void mark_none() { dirty.assign((size_t)tree.nnodes() * 3, 0); }
};

void det_record(int batch, const Gene &G, char kind, int a, int b, double x, double y, double z);   // PML_DET_LOG diagnostic (engine.cpp)
double now_ms();                      // host wall clock (launch.cpp)
inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

struct pml_alignment_view { int ntax, nsites; const char *const *names; const char *const *rows; };

// gene alignments encoded ONCE and kept in HBM; replicates (gene subsets) are gathered from them on the device
struct GeneStore {
    struct Item { EncodedAlignment aln; std::vector<int64_t> cmp, diff; uint8_t *d_codes = nullptr; double *d_w = nullptr; };
    Ctx *ctx = nullptr; std::vector<Item> items; char *arena = nullptr;
    int create(Ctx *c, int n, const pml_alignment_view *alns);
    void destroy();
};

constexpr int NNI_PARTS = 6;         // parts an NNI round deals a gene's edges over (four scratch CLVs each)
constexpr int NSCRATCH = 4 * NNI_PARTS > 8 ? 4 * NNI_PARTS : 8;   // extra CLV slots per gene for candidate evaluation (NNI: 4 per part; SPR: 8)
enum { SIDE_TIP = 0, SIDE_MSG = 1, SIDE_SCRATCH = 2, SIDE_CHERRY = 3, SIDE_PITCH = 4 };
// tip node id | directed-edge index (v-ntax)*3+k | scratch slot | directed-edge index of a message whose
// two children are tips ("cherry": never materialised, recomputed from two tip tables where consumed)
struct Side { int kind, id; };
// bv/bq (optional, scratch outputs): the tree branch (node, slot) child c's length belongs to -- lets run() share ONE
// transition-matrix request among all operations of a launch that cross the same branch
struct PendingOp { int gene, out_kind, out_id, level; Side child[2]; double t[2]; int bv[2] = {-1, -1}, bq[2] = {0, 0};
                   bool unstored = false; /* run(): the result stayed in registers (OPF_NO_STORE) and is not valid in memory */
                   bool transient = false; /* caller: only the operation or tail that directly follows reads the result (scratch slots) */
                   int part = 0; /* run(): operations and tails of one gene with different parts are independent of each other and become separate runs
                                    of the launch (their workgroups run side by side): NNI rounds deal the edges of a gene over parts */ };

// One set of launches (k_pmat, k_oplist, k_reduce, then k_newton or its SEQ form) as run() lays it out in a staging block.
// A deferred step of a chained pass and a recorded scoring plan are each one of these; Batch::issue() launches it.
struct LaunchSet {
    size_t o_req = 0, o_ops = 0, o_runs = 0, o_red = 0, o_newt = 0, o_tick = 0, bytes = 0;   // offsets of the six arrays (multiples of 256), size of the block
    size_t nreq = 0, nruns = 0, neval = 0; int nt_reg = 0, nt_stream = 0;   // matrix requests, k_oplist runs, reductions, k_newton tickets (register / streaming form)
    bool seq = false, fused = false;                // Newton through the no-exchange SEQ form; k_oplist has fused Newton tails
    bool any_pitch = false, any_chain = false; int max_mpad = 0; double algo_bytes = 0, algo_flops = 0, newton_bytes = 0;    // SURVEY 8d accounting
};
// pml_search2: one accepted step of a gene's search, and the record of the whole search (peprml.h pml_search_trace)
struct SearchStep { int phase, rmin, rmax, distance; double lnl_before, lnl_after; std::string newick_after; };
struct SearchTrace { int radius_chosen = 0; std::vector<int> trial_radius; std::vector<double> trial_lnl; double lnl_start = 0; std::vector<SearchStep> steps; };
struct Search2Opts { bool nni = true, opt_alpha = true; double eps = 1e-3; bool radius_auto = false; int radius = 0, radius_step = 5, radius_max = 25;
                     bool thorough = false; int thorough_top = 0, thorough_radius_max = 20; };
// one thorough insertion: the subtree cut off by prune (p, ks) of gene g regrafted into the candidate's edge with the pendant
// branch ts and the two halves tg, th of the split edge optimised (in: start values; out: what the sweeps settled on), score =
// the lnL of that tree with nothing else touched
struct ThoroughJob { int g, p, ks; SprCandidate cand; double ts, tg, th, score; int sweeps; };
struct BootSet; struct BootDebug;    // boot_dev.hpp / below: the column bootstrap
struct Batch {
    Ctx *ctx = nullptr;
    int pi_mode = 0, ncat = 4, det_id = 0;
    const ModelDev *d_shared = nullptr; const double *d_shared_eig = nullptr;      // the context's model of a shared code
    // per-gene models (model_per_gene codes, genes of different codes, or after set_matrix): every gene has its own eigen-system
    ModelDev *d_gmodel = nullptr; double *d_geig = nullptr;       // [genes] models, [genes][2*PFRAG] eigen-basis fragment sets
    // what the genes' models are built from, device copies read by k_model and pinned host mirrors: [genes][190], [genes][20]
    double *d_gexch = nullptr, *d_gpi = nullptr, *h_gexch = nullptr, *h_gpi = nullptr;
    ModelReq *d_mreq = nullptr, *h_mreq = nullptr;                // [genes] build requests
    ModelDev *h_gmodel = nullptr;                                 // [genes], PML_MODEL_HOST=1 only: the host-built A/B arm of build_models
    const ModelDev *model_of(int g) const { return d_gmodel ? d_gmodel + g : d_shared; }
    const double *eig_of(int g) const { return d_geig ? d_geig + (size_t)g * 2 * PFRAG : d_shared_eig; }
    int alloc_gene_models();
    int build_gene_models();
    // the exchangeabilities and (normalised) frequencies gene g's code stands for (empirical frequencies counted from its alignment)
    void matrix_for(int g, double *exch190, double *pi20) const;
    void empirical_pi(int g, double *pi20) const;       // gene g's counted frequencies: from its text, or from its device histogram
    int count_replicate_freqs();                        // k_codehist over every gene of a gathered batch -> code_hist, counted_pi
    // k_model + k_eigfrags for the listed genes from d_gexch / d_gpi; patch >= 0: rate `patch` of gene gs[i] counts as vals[i]
    int build_models(const std::vector<int> &gs, int patch, const double *vals);
    int set_matrix(int g /* -1 = all */, const double *exch190, const double *pi20 /* null = keep */);
    int get_matrix(int g, double *exch190, double *pi20) const;
    // PROTGAMMAGTR: one sweep over the 189 free rates of every active GTR gene, each by Brent on its logarithm, genes in lock step
    int opt_rates(const std::vector<char> &active, double *lnl, double tol);
    bool rates_on = true;          // optimize() estimates the rates of GTR genes (a search holds them fixed between its first and last optimisation)
    long cnt_rate_trials = 0;
    int spr_scratch_radius = 0;    // set before create(): the largest SPR radius the batch will search (search2 batches; 0 = NSCRATCH serves)
    int share = 1;                 // batches working on the device at the same time (groups of one search call): free HBM is divided by it
    double newton_tol = 1e-8;      // Newton stop |dt| < tol: 1e-8 fine, 1e-6 in coarse phases
    std::vector<Gene> genes;
    char *arena = nullptr; size_t arena_bytes = 0;
    // staging (pinned host mirrors + device buffers), grown on demand
    void *h_stage = nullptr; size_t h_cap = 0;
    void *d_stage = nullptr; size_t d_cap = 0;
    double *d_frags = nullptr; size_t frag_cap = 0;      // in fragment sets
    double *d_scalars = nullptr; double *h_scalars = nullptr;   // 8 doubles per gene and tail slot: device buffer + pinned host mirror
    size_t scalars_doubles = 0, results_used = 0;
    double *h_plan_lnl = nullptr, *d_plan_lnl = nullptr;         // replayed scoring plans: one lnL per gene in mapped pinned memory (host pointer, device address)
    int fetch_results(bool pooled);                              // enqueue the device -> host copies of the result buffers
    double *d_nsync = nullptr; size_t nsync_cap = 0;             // Newton inter-workgroup sync blocks
    NewtonCtl *d_nctl = nullptr;                                  // k_newton's control block (tickets, abort word)
    // k_newton's exchange gave up (a co-tenant kept slices of a request apart for longer than the wall-clock bound): the
    // affected work is re-issued through the no-exchange SEQ form, and the next `safe_left` Newton launch sets use it from the
    // start (doubling hold-off, so a GPU that stays shared costs one time-out per hold-off period, not one per launch)
    int safe_left = 0, safe_hold = 4; bool safe_now = false;
    unsigned newton_launch_seq = 0;      // launches with Newton tails so far: the exchange granules' tag base (never cleared, tags are unique)
    bool in_retry = false;
    bool newton_safe_mode() { return safe_now || safe_left > 0; }
    void newton_gave_up();
    int clear_abort();
    // cached descriptors of the full-traversal score of ALL genes (topology unchanged): replays skip
    // the tree walk and the descriptor build; transition matrices, CLVs and lnL are recomputed
    struct ReqSrc { int gene, v, q, fold; };      // branch (v, slot q) whose length a P request uses
    struct Plan {
        bool valid = false; unsigned epoch = 0;
        void *h = nullptr, *d = nullptr; size_t cap = 0;     // pinned host and device copy of the recorded staging block
        LaunchSet set;
        bool stored = false;                       // recorded with every CLV written (the traversal a search runs) instead of OPF_NO_STORE
        std::vector<ReqSrc> src; std::vector<std::pair<int, int>> outs;
        std::vector<unsigned> rates_seen;          // per gene: rates_epoch the descriptors carry
        std::vector<unsigned long long> len_seen;  // per gene: Tree::len_stamp of the branch lengths the descriptors carry (0: not compared yet)
        // PML_CHECK_LEN_STAMP=1 when the plan was recorded (test hook): every replay also compares the lengths as bytes against
        // this copy per gene and fails if they differ under an unchanged stamp
        bool check_len = false; std::vector<std::vector<std::array<double, 3>>> len_copy;
        std::vector<char> moved;                   // replay scratch, per gene: bit 0 lengths, bit 1 rates differ from the descriptors
        bool per_gene = false;                     // one evaluation per gene in gene order: the reductions write d_plan_lnl
    } plan;
    long cnt_smooth = 0, cnt_nni = 0, cnt_spr = 0, cnt_eval = 0, cnt_passes = 0;   // run() calls by purpose (PML_TRACE)
    // host wall time by phase, ms (PML_TRACE prints them at the end of a search): where the device waits for the host
    enum { HP_PASS_SETUP, HP_PASS_STEPS, HP_PASS_SYNC, HP_PASS_POST, HP_NNI_BUILD, HP_NNI_RUN, HP_NNI_SELECT, HP_ALPHA_HOST, HP_RUN_SYNCED, HP_N };
    double host_phase_ms[HP_N] = {0};
    unsigned topo_epoch = 0;       // bumped whenever a search may change a topology
    bool score_only_batch = false;
    int replay_plan(double *lnl);
    bool record_plan = false, record_stored = false;
    // run()'s scratch, kept between launches: the device waits while descriptors are built, so a launch allocates nothing
    struct LaunchScratch {
        std::vector<size_t> req_off; std::vector<uint32_t> req_stamp; std::vector<const double *> req_ptr; uint32_t req_launch = 0;   // keyed request table
        std::vector<std::vector<std::pair<uint64_t, const double *>>> val_bucket; std::vector<uint32_t> val_stamp;   // requests shared by value
        std::vector<std::vector<int>> run_tails_of; std::vector<int> run_nparts; std::vector<size_t> run_koff;       // tails, parts and first run key per gene
        std::vector<ReqSrc> last_src; std::vector<char> fused_req; std::vector<int> tail_req;   // [request] its branch; [Newton request] fused; [tail] its Newton request or -1
    } scratch;
    std::vector<std::vector<std::pair<int, int>>> pass_order; std::vector<std::vector<uint8_t>> pass_next;      // smooth_pass scratch
    // chained mode: run() enqueues its copy + kernels and returns WITHOUT synchronising; descriptors are bump-
    // allocated in the staging buffer; branch lengths optimised earlier in the chain are read from Gene::d_len
    bool chain = false; size_t chain_off = 0;
    double *d_lenpool = nullptr;
    double *d_chain = nullptr, *h_chain = nullptr; size_t chain_cap = 0;     // 4 doubles per chained Newton result
    // a step of a chained pass whose upload + launches are issued later, grouped with its neighbours (flush_deferred)
    struct Deferred { LaunchSet set; size_t base; /* of its block in the staging ring */ }; std::vector<Deferred> deferred; size_t flush_quota = 1;
    int flush_deferred();
    // the launches of one set from its block at ds (device memory); self_timed: as a replayed plan, else as a flushed step
    void issue(const LaunchSet &L, const char *ds, bool self_timed);
    int chain_begin(size_t nresults);
    int ensure_results(size_t nresults);   // d_chain (device) / h_chain (pinned mirror): 4 doubles per pooled result
    // pooled sumtables for launches that carry more Newton requests per gene than MAXTAIL (all edges of an NNI round)
    char *d_tailpool = nullptr; size_t tailpool_cap = 0;
    int ensure_tailpool(size_t bytes);
    int chain_sync();                  // wait for everything enqueued; the staging buffer is free again

    int create(Ctx *c, int n, const pml_alignment_view *alns, const char *const *newicks,
               int pi_mode, int ncat, double alpha, bool score_only, const int *gene_codes = nullptr /* a code per gene instead of pi_mode */);
    // one batch gene per replicate = the concatenation of the selected store genes (sorted taxon union, absent
    // taxa = gap rows, MSAConcatenator rules); code matrices are gathered on the device, NJ start trees come from
    // the summed pair counts: no column text is touched again.  A per-gene code (empirical frequencies, GTR) gives every
    // replicate its own model, its frequencies counted on the device (k_codehist)
    int create_replicates(Ctx *c, const GeneStore &store, const std::vector<std::vector<int>> &sel, int pi_mode, int ncat, double alpha);
    // the counterpart for the column bootstrap (boot.cpp): one batch gene per replicate [reps_begin, reps_end) of the call with
    // `seed` over the concatenation of the selected store genes.  A replicate is the patterns its draws hit, compacted in
    // ascending order, each weighted by its number of draws (boot.hpp); count, index, read-back of the pattern counts, layout,
    // gather, pair counts and NJ starts, all from the resident genes.  set: the selection's column space when the caller keeps
    // one for several sub-batches (null = built here); dbg: replicate reps_begin's idx and pair counts for the test door
    int create_bootstrap(Ctx *c, const GeneStore &store, const std::vector<int> &sel, int reps_begin, int reps_end, unsigned long long seed,
                         int pi_mode, int ncat, double alpha, const struct BootSet *set = nullptr, struct BootDebug *dbg = nullptr);
    int layout(double alpha, bool score_only);
    void destroy();

    void set_alpha(int g, double alpha);
    void invalidate_all(int g);
    void branch_changed(int g, int a, int b);
    // lnL of every active gene at the branch above taxon 0, using/refreshing cached CLVs
    int evaluate(const std::vector<char> &active, double *lnl);
    // invalidate + evaluate; stored: the whole-tree pass writes every CLV (chained children are still READ from registers),
    // i.e. the traversal a search runs after a topology or alpha change -- bench.py's second timed leg
    int score(const std::vector<char> &active, double *lnl, bool stored = false);
    int site_lnl(int g, double *out);
    int root_derivs(double *lnl, double *d1, double *d2);
    // one pass over the DIRTY branches (DFS order); a branch that moves by more than thr flags itself and
    // its neighbours for the next pass
    int smooth_pass(const std::vector<char> &active, std::vector<double> &maxdelta, double thr);
    int opt_alpha(const std::vector<char> &active, double *lnl, double tol = 1e-4);
    int optimize(bool opt_alpha_flag, double eps, double *lnl, const std::vector<char> *mask = nullptr);
    int light_smooth(const std::vector<char> &active, double *lnl);
    int nni_round(const std::vector<char> &active, std::vector<double> &lnl, std::vector<int> &applied);
    int spr_round(const std::vector<char> &active, int radius, std::vector<double> &lnl, std::vector<int> &moves);
    int search(bool nni, int spr_radius, bool opt_alpha_flag, double eps, double *lnl);
    // the lazy SPR round with a radius per gene and a distance window [rmin, radius]; radii beyond what the gene's scratch
    // slots serve are cut to that; trace (optional, per gene): every kept move is appended as a phase-1 step
    int spr_round_windowed(const std::vector<char> &active, const std::vector<int> &radius, int rmin, std::vector<double> &lnl,
                           std::vector<int> &moves, std::vector<SearchTrace> *trace);
    // RAxML's schedule (peprml.h pml_search2): radius determination, fast phase, final optimisation
    int search2(const Search2Opts &o, double *lnl, std::vector<SearchTrace> *trace);
    // test door: the lazy scores of the candidates of one prune of gene 0, in spr_candidates' order, and the thorough
    // insertions of the thorough_top best of them (0 = none, < 0 = all): thorough[i] = {score, ts, tg, th} or NaNs
    int spr_scores(int p, int ks, int rmin, int rmax, int thorough_top, std::vector<SprCandidate> &cands, std::vector<double> &lazy,
                   std::vector<std::array<double, 4>> &thorough);
    // Gauss-Seidel Newton over the three branches of every job (<= 8 sweeps, stop when a sweep moves no length by more than
    // newton_tol), then its evaluation; all jobs of all genes advance in lockstep, one launch set per Newton
    int thorough_insert(std::vector<ThoroughJob> &jobs);
    // one cycle of the thorough phase: every prune of every active gene, candidates within the gene's window
    int thorough_cycle(const std::vector<char> &active, const std::vector<int> &rmin, const std::vector<int> &rmax, int top,
                       std::vector<double> &lnl, std::vector<int> &moves, std::vector<SearchTrace> *trace);
    // SH-like local supports (FastTree's default output; FastTreeRunner.java:67-70 without -nosupport): per gene one value
    // per internal edge in nni_round's edge order (u ascending, slot ascending, v > u inner), plus the (u, v) pairs
    // FastTree -gamma: per-pattern likelihoods at the 20 fixed rates (five traversals of four rates), then alpha and the
    // length rescale fitted on that table (k_g20 evaluates, the host steers two alternating Brent searches per gene)
    int gamma20(std::vector<double> &lnl20, std::vector<double> &alpha20, std::vector<double> &rescale20);
    int sh_support(int nboot, unsigned long long seed, std::vector<std::vector<double>> &support, std::vector<std::vector<std::pair<int, int>>> &edges_out);
    int *d_site2pat = nullptr; std::vector<size_t> site2pat_off;
    // FastTree -constraints matrix (names, rows of '0' '1' '-'); start trees that violate it are rebuilt
    int set_constraints(int ncons, int ntax, const char *const *names, const char *const *rows);

    // --- plumbing ---
    int need(int g, int v, int to, std::vector<PendingOp> &ops);   // returns level
    // run the collected newviews, then the tail ops (evaluate or sumtable+newton), one sync
    // a tail is evaluated after `after` newview ops of its gene (-1 = after all of them); `slot`
    // selects one of the gene's MAXTAIL sumtable / per-pattern-lnL / result buffers
    struct Tail { int gene; Side a, b; int mode; double t0; int max_iter; int slot = 0; int after = -1;
                  int bv = -1, bq = 0; /* tree branch (node, slot) t0 comes from: plan replay */
                  double *result_dev = nullptr;               /* chained pass: where k_newton writes (else res(g, slot)) */
                  double *t_dev0 = nullptr, *t_dev1 = nullptr; /* chained pass: d_len entries of the branch */
                  double *patlnl_dev = nullptr;               /* Newton tails: per-pattern lnL at the optimised length */
                  double *sumtab_dev = nullptr;               /* Newton tails: pooled sumtable (80*mpad doubles + mpad ints) instead of the gene's slot buffer */
                  int *scl_dev = nullptr;                     /* MODE_EVALUATE_CAT: where the scaling counts go (patlnl_dev = the 4 x mpad table slice) */
                  const double *result_host = nullptr;        /* host view of result_dev when it is mapped memory (checked after the sync) */
                  int part = 0;                               /* as PendingOp::part */ };
    double *res(int g, int slot = 0) const { return h_scalars + 8 * ((size_t)g * MAXTAIL + slot); }
    Side msg(int g, int node, int toward) const;
    bool is_cherry(int g, int node, int toward) const;
    // 0: real message, 1: cherry (two tips), 2: pitchfork (a cherry and a tip): both are virtual
    int virt_kind(int g, int node, int toward) const;
    bool virtual_pitch = true;         // PML_NO_PITCH=1
    bool virtual_cherries = true;      // PML_NO_CHERRY=1 materialises cherry CLVs like any other (A/B switch)
    int run(std::vector<PendingOp> &ops, const std::vector<Tail> &tails);
    int ensure_stage(size_t bytes);
    int ensure_frags(size_t sets);
    int slot_for(Gene &g, int idx);
};

// parsimony.hip: Fitch parsimony trees (stepwise addition + SPR) for n genes, one launch per device step
int parsimony_batch(Ctx *ctx, int n, const pml_alignment_view *alns, unsigned seed, int radius, std::vector<Tree> &trees_out,
                    std::vector<EncodedAlignment> &alns_out, std::vector<long long> &lengths_out, std::vector<int> &moves_out);
// the same trees for gene selections over a resident store (the jackknife): tip vectors straight from the genes' code matrices
// (k_fitch_tips, one launch for all selections), a seed per selection; names_out[r] = the selection's sorted taxon union
int parsimony_replicates(Ctx *ctx, const GeneStore &store, const std::vector<std::vector<int>> &selections, const std::vector<unsigned> &seeds,
                         int radius, std::vector<Tree> &trees_out, std::vector<std::vector<std::string>> &names_out, std::vector<long long> &lengths_out);
// test door: the tip rows [ntax x mpad] and weights [mpad] k_fitch_tips writes for one selection
int fitch_tips_readback(Ctx *ctx, const GeneStore &store, const std::vector<int> &sel, int *npat_out, int *mpad_out, std::vector<unsigned> &masks_out,
                        std::vector<int> &weights_out, std::vector<std::string> &names_out);

// the column bootstrap's parsimony trees (parsimony.hip): replicates [reps_begin, reps_end) of the call with `seed` over the
// selection's column space, their tip rows and weights written by k_boot_gather; replicate r gets the stepwise-addition seed
// boot_parsimony_seed(seed, 1 + r).  All replicates cover set.names
int parsimony_bootstrap(Ctx *ctx, const struct BootSet &set, int reps_begin, int reps_end, unsigned long long seed, int radius,
                        std::vector<Tree> &trees_out, std::vector<long long> &lengths_out);
// test door: the tip rows [ntax x mpad] and weights [mpad] of one bootstrap replicate
int boot_tips_readback(Ctx *ctx, const struct BootSet &set, int rep, unsigned long long seed, int *npat_out, int *mpad_out,
                       std::vector<unsigned> &masks_out, std::vector<int> &weights_out);
struct BootDebug { std::vector<int> idx; std::vector<int64_t> cmp, diff; };

}  // namespace pml
