/*
 * peprml.h -- C ABI of libpeprml.so, the MI355X-native maximum-likelihood tree engine that
 * replaces the external-process calls on PEPR's tree-building path.
 *
 * Every entry point names the reference interface it replaces (paths relative to the PEPR
 * repository, src/edu/vt/vbi/ci/ abbreviated as .../):
 *
 *   pml_score      <- .../pepr/tree/RAxMLRunner.java:162-213   runRaxmlPerSiteLL():
 *                        `raxmlHPC -f g -m PROTGAMMAWAG -z trees -s aln` -> RAxML_perSiteLLs.<run>
 *   pml_optimize   <- .../pepr/tree/FastTreeRunner.java:142-199 getRaxmlBranchLengths() and
 *                     .../pepr/tree/RAxMLRunner.java:253-272:  `raxmlHPC -f e -t tree` -> RAxML_result.<run>
 *   pml_search     <- .../pepr/tree/RAxMLRunner.java:79-152     run():  `raxmlHPC -f d -m PROTGAMMAWAG`
 *                     .../pepr/tree/FastTreeRunner.java:38-135  run():  `FastTree_WAG -gamma -nosupport`
 *   pml_*_batch    <- .../pepr/tree/pipeline/PhylogenomicPipeline2.java:1587-1633
 *                        GeneSubsetTreeRunnable.run(): the data-parallel loop of independent tree builds
 *   pml_rf_distance<- .../pepr/tree/AdvancedTree.java:1460-1491 (Robinson-Foulds used for acceptance)
 *   pml_tree_compare<- .../pepr/tree/TreeComparison.java:267-288 compareAllvsAll(): legacy RF (Tree.java:589-603), the two
 *                        branch distances (:607-810) and AdvancedTree's RF for every pair of a tree set, ONE call
 *   pml_jackknife  <- .../pepr/tree/pipeline/PhylogenomicPipeline2.java:994-1126
 *                        buildConcatenatedTreeWithGeneWiseJackKnifeSupport(): full tree + N support trees on
 *                        random gene subsets (:959-977, 1227-1275, 1587-1633) + support counts, ONE call
 *   pml_jackknife3 <- the same loop with `-full_tree_method` / `-support_tree_method` parsimony (:856-863, :1246, :1619)
 *   pml_parsimony  <- .../pepr/tree/RAxMLRunner.java:215-251  runRaxmlParsimonyWithBranchLengths():
 *                        `raxmlHPC -f d -y` -> RAxML_parsimonyTree.<run> (topology only); the caller then
 *                        runs pml_optimize on it, as the reference runs `-f e -t` (:253-272)
 *   pml_bootstrap  <- .../pepr/tree/RAxMLRunner.java:115-132,302-318 (`-f a -x -N`, bootstrapReps > 0)
 *   pml_sh_support <- .../pepr/tree/FastTreeRunner.java:67-70 (`FastTree_WAG -gamma` without -nosupport)
 *   pml_gamma20    <- .../pepr/tree/FastTreeRunner.java:67-70 (`-gamma`: the "Gamma(20) LogLk ... alpha ... rescaling
 *                        lengths" step that ends every FastTree_WAG run PEPR makes; its printed tree is what PEPR parses)
 *   pml_concatenate<- .../pepr/alignment/MSAConcatenator.java:78-189 (sorted taxon union, '?' padding)
 *   pml_refine_next<- .../pepr/tree/PhylogeneticTreeRefiner.java:298-359 + AdvancedTree.java:1061-1098
 *   pml_support_tree<- .../pepr/tree/TreeSupportDecorator.java:86-163 addSupportValues(): integer
 *                        bipartition counts of the support trees written as node labels of the main tree
 *   pml_nj_tree    <- .../pepr/tree/pipeline/PhylogeneticTreeBuilder.java:198-208 buildNeighborJoiningTree() (method `nj`) and
 *                        .../pepr/tree/pipeline/PhylogenomicPipeline2.java:1279-1293 buildConcatenatedNeighborJoiningTree() (`-nj true`):
 *                        SequenceAlignment.getPairwiseScores (BLOSUM62 as AlignmentUtilities loads it), then
 *                        TreeBuilder.getNJTreeString / getNJTopology; pml_nj_jackknife is the gene-wise jackknife with
 *                        `-full_tree_method nj -support_tree_method nj`
 *   pml_tree_tests <- .../pepr/tree/TreeComparison.java:812-885 runConsel(): `raxmlHPC -f g -z trees` piped through
 *                        `makermt -b 10 --puzzle`, `consel`, `catpv -v` -> the table of AU / KH / SH / bootstrap p-values;
 *                        pml_rell_tests is the makermt | consel | catpv half alone, on a per-site lnL table the caller has
 *
 * Conventions: caller owns inputs (nothing is retained after return);
 * the library allocates results, the caller releases them with pml_result_free(); no files, no
 * cwd dependence, no stdout/stderr output; every function returns 0 or a negative PML_E* code and
 * never aborts or throws.  A context may be used from several threads: batch calls serialise on it,
 * concurrent single-gene calls are coalesced into one device batch (pml_coalescing_stats).
 * The alignment rows are exactly SequenceAlignment.alignedSequenceChars
 * (.../pepr/alignment/SequenceAlignment.java:61): one char row per taxon, 20 amino-acid letters,
 * '-' gap, '?' absent gene, anything else unknown (treated like a gap; B/Z are N|D and Q|E).
 *
 * There is NO CPU fallback: without a HIP device pml_create() fails with PML_ENODEVICE.
 */
#ifndef PEPRML_H
#define PEPRML_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define PML_OK          0
#define PML_EINVAL     -1   /* bad argument */
#define PML_EPARSE     -2   /* Newick / alignment parse error (message in pml_last_error) */
#define PML_ENODEVICE  -3   /* no usable HIP device */
#define PML_ENOMEM     -4   /* host or device allocation failed */
#define PML_EDEVICE    -5   /* HIP runtime error */
#define PML_ENOTFOUND  -6

typedef struct pml_ctx pml_ctx;
typedef struct pml_batch pml_batch;

typedef struct {
    int device;              /* HIP device ordinal (rank-local GPU) */
    int profile;             /* 1: record HIP events around kernels (pml_kernel_stats) */
    size_t arena_bytes;      /* > 0: reserve this much HBM at pml_create for batch arenas (a fresh allocation is
                              * zero-filled by the driver at ~40 GB/s); 0 = allocate per batch, keep the last one */
} pml_config;

typedef struct {
    int ntax;
    int nsites;
    const char *const *names;   /* ntax taxon names (Newick leaf labels) */
    const char *const *rows;    /* ntax rows of nsites chars */
} pml_alignment;

/* PML_PI_EMPIRICAL = RAxML's "F" models (PROTGAMMAWAGF, one of the names -matrix_eval passes, PhylogenomicPipeline2.java:260-284;
 * RAxMLRunner's own default is an F model, RAxMLRunner.java:46): WAG exchangeabilities with frequencies counted from each
 * gene's alignment (eight sweeps of proportional counting, ambiguity codes spread over their states, floor 0.001) -- a
 * per-gene eigen-system.  Built for score / optimize / search / per-site calls and resident batches; the jackknife's
 * device-gathered replicates refuse it. */
enum { PML_PI_RAXML_3DP = 0, PML_PI_WAG_FULL = 1, PML_PI_EMPIRICAL = 2,
       /* RAxML's PROTGAMMAGTR: the 189 free exchangeabilities of the gene are estimated by maximum likelihood (the 190th is
        * fixed at 1), frequencies empirical.  The optimising calls (pml_optimize*, pml_search*, pml_batch_optimize,
        * pml_batch_search, pml_model_eval) estimate them; a call that does not optimise scores a gene whose matrix was never
        * set or estimated under the start matrix, WAG's exchangeabilities -- documented behaviour, not an error. */
       PML_PI_GTR = 3,
       /* pml_matrix_register returns codes from here on: `code` (even) = the registered matrix with its own frequencies, one
        * shared model; `code + 1` = its exchangeabilities with each gene's empirical frequencies (RAxML's "F" variant). */
       PML_PI_REGISTERED = 16 };

typedef struct {
    int ncat;                /* Gamma categories (4 = RAxML PROTGAMMA; 1 = no rate heterogeneity) */
    double alpha;            /* Gamma shape (start value when optimised) */
    int pi_mode;             /* the model: PML_PI_RAXML_3DP (RAxML 7.2.5 PROTGAMMAWAG), PML_PI_WAG_FULL (FastTree_WAG), PML_PI_EMPIRICAL
                              * (PROTGAMMAWAGF), PML_PI_GTR (PROTGAMMAGTR) or a code of pml_matrix_register */
} pml_model;

typedef struct {
    int optimize_alpha;      /* 1: Brent on alpha */
    int nni;                 /* 1: NNI hill climbing */
    int spr_radius;          /* >0: SPR rounds with this rearrangement radius.  pml_search, pml_search_batch, pml_batch_search,
                              * pml_bootstrap and pml_jackknife* search at most radius 6: a larger value is cut to 6 without
                              * an error (kept for the bits of existing callers); pml_search2 honours radii up to 25 */
    double epsilon;          /* stop when a round gains less than this many lnL units */
    unsigned seed;           /* 0: NJ start tree (deterministic); != 0: randomised stepwise-addition parsimony start with
                              * this seed, as `raxmlHPC -f d -p seed` starts (genes that come with a start tree keep it) */
    /* topological constraints, FastTree's -constraints semantics as PEPR produces them
     * (FastTreeRunner.getFastTreeConstraintsForTree, FastTreeRunner.java:243-273): a 0/1/- matrix,
     * one row per named taxon, one column per constrained split ('-' = taxon free in that column).
     * The result tree displays every non-trivial column; taxa absent from the matrix are free.
     * nconstraints = 0: unconstrained. */
    int nconstraints;
    int constraint_ntax;
    const char *const *constraint_names;
    const char *const *constraint_rows;
} pml_search_opts;

typedef struct {
    int status;              /* PML_OK or error for this gene */
    double lnl;              /* log likelihood */
    double alpha;            /* Gamma shape used / found */
    double tree_length;      /* sum of branch lengths */
    int npatterns;           /* alignment patterns after compression */
    int nsites;
    char *newick;            /* resulting tree, NUL-terminated, RAxML-style unrooted (may be NULL) */
    double *site_lnl;        /* per-site lnL in alignment column order (only if requested) */
} pml_result;

#define PML_WANT_SITE_LNL 1   /* flags for pml_score */

/* lifecycle */
int  pml_create(const pml_config *cfg, pml_ctx **out);
void pml_destroy(pml_ctx *ctx);
const char *pml_strerror(int code);
const char *pml_last_error(pml_ctx *ctx);     /* detail of the last failure on this context */
const char *pml_version(void);

/* one-shot calls (one gene) */
int pml_score(pml_ctx *ctx, const pml_alignment *aln, const char *newick, const pml_model *model,
              int flags, pml_result *out);
int pml_optimize(pml_ctx *ctx, const pml_alignment *aln, const char *newick, const pml_model *model,
                 const pml_search_opts *opts, pml_result *out);
int pml_search(pml_ctx *ctx, const pml_alignment *aln, const char *start_newick /* NULL = NJ */,
               const pml_model *model, const pml_search_opts *opts, pml_result *out);

/* gene-batched calls: n independent (alignment, tree) units evaluated together on the device */
int pml_score_batch(pml_ctx *ctx, int n, const pml_alignment *alns, const char *const *newicks,
                    const pml_model *model, int flags, pml_result *out);
int pml_optimize_batch(pml_ctx *ctx, int n, const pml_alignment *alns, const char *const *newicks,
                       const pml_model *model, const pml_search_opts *opts, pml_result *out);
int pml_search_batch(pml_ctx *ctx, int n, const pml_alignment *alns, const char *const *start_newicks,
                     const pml_model *model, const pml_search_opts *opts, pml_result *out);
void pml_result_free(pml_result *r);

/* RAxML's search schedule (`raxmlHPC -f d`, RAxMLRunner.java:115-147): radius determination on the start tree, fast lazy SPR
 * cycles at that radius, final optimisation.  These are this project's definitions, written from RAxML's published algorithm
 * (Stamatakis 2006, "RAxML-VI-HPC"); RAxML's source is not part of the reference, so parity with RAxML's own trees is NOT
 * pinned, as everywhere else.
 *   start     as pml_search: constraints check, coarse optimisation (epsilon 0.1) -> tree T0, lnL L0 = trace lnl_start
 *   radius    FIXED: base.spr_radius, honoured up to PML_SPR_RADIUS_MAX (no clamp at 6; larger = PML_EINVAL).
 *             AUTO: for r = step, 2 step, ... <= radius_max: from a copy of T0 one lazy SPR round at radius r, then the coarse
 *             optimisation, L_r recorded; stop after the first r whose L_r does not exceed the best so far (L0 counts); the
 *             radius is the first r that reached the maximum (radius_step if none beat L0) and the search goes on from that
 *             trial's tree (from T0 if none).  In a batch every gene determines its own radius and stops on its own.
 *   fast      pml_search's loop with the gene's radius: NNI rounds if base.nni, lazy SPR rounds, coarse optimisation, until
 *             a pass applies no move.  base.nni = 0 is honoured: no NNI round runs (pml_search runs them in front of its
 *             SPR rounds whatever nni says once spr_radius > 0, so the two calls differ for nni = 0 with a radius).
 *   thorough  (thorough = 1, after the fast phase) distance windows [1, step], [step + 1, 2 step] ...: in a cycle every prune
 *             scores the candidates whose distance lies in the window lazily; the thorough_top best get the thorough
 *             insertion -- Gauss-Seidel Newton over the pendant branch and the two halves of the split edge at the search's
 *             Newton tolerance (1e-6), until a sweep moves no length by more than that, 8 sweeps at most, then an evaluation;
 *             the best thorough score is applied if it beats the current lnL by 0.01 and then goes through the lazy move's
 *             apply phases (four branch Newtons, kept only if the tree really improved) from the three lengths found.  A
 *             cycle without an accepted move shifts the gene's window by step, one with a move resets it to [1, step]; the
 *             phase ends when the window's upper edge would pass thorough_radius_max.
 *   end       optimisation to base.epsilon (0 = 1e-3), rates of PML_PI_GTR re-estimated, as pml_search
 * Constraints apply at every radius.  A gene's result and trace are a function of the gene and the options alone, bit for bit,
 * whatever shares its batch.  With radius_mode FIXED, base.spr_radius <= 6, base.nni = 1 and thorough 0 the call returns
 * pml_search's bits.
 * Radii above 22 need more scratch CLVs than other batches carry: a batch created by these calls gets them (min(radius,
 * ntax) + 2 per gene), and they count in its HBM bound.  RAxML's lnL cut-off during the descent is not built: every
 * candidate of a prune is scored in one launch. */
#define PML_SPR_RADIUS_MAX 25
enum { PML_RADIUS_FIXED = 0, PML_RADIUS_AUTO = 1 };
typedef struct {
    pml_search_opts base;     /* optimize_alpha, nni, epsilon, seed, constraints: pml_search's meaning */
    int radius_mode;          /* FIXED: base.spr_radius (0 .. PML_SPR_RADIUS_MAX); AUTO: determined on the start tree, base.spr_radius is not used */
    int radius_step;          /* AUTO and the thorough windows; 0 = 5 */
    int radius_max;           /* AUTO; 0 = 25; step <= radius_max <= PML_SPR_RADIUS_MAX */
    int thorough;             /* 1: thorough phase after the fast phase */
    int thorough_top;         /* candidates of a prune that get the thorough insertion, best lazy scores first; 0 = all */
    int thorough_radius_max;  /* last window's upper edge; 0 = 20; <= PML_SPR_RADIUS_MAX */
} pml_search_opts2;
typedef struct {              /* one accepted step */
    int phase;                /* 0 = an NNI round (one entry per round that applied moves), 1 = lazy SPR move, 2 = thorough SPR move */
    int rmin, rmax;           /* the window the move was found in (phase 0: 0, 0) */
    int distance;             /* SPR: edges from the joined edge at the pruning point to the regraft edge, that edge included */
    double lnl_before, lnl_after;
    char *newick_after;       /* the tree after the step and its branch Newton, 12 digits */
} pml_search_step;
typedef struct {
    int radius_chosen, ntrials; int *trial_radius; double *trial_lnl;   /* AUTO; FIXED: the given radius, ntrials 0 */
    double lnl_start;         /* after the first optimisation of the start tree */
    int nsteps; pml_search_step *steps;
} pml_search_trace;
int pml_search2(pml_ctx *ctx, const pml_alignment *aln, const char *start_newick /* NULL = NJ / parsimony */, const pml_model *model,
                const pml_search_opts2 *opts, pml_result *out, pml_search_trace *trace /* NULL ok */);
int pml_search2_batch(pml_ctx *ctx, int n, const pml_alignment *alns, const char *const *start_newicks, const pml_model *model,
                      const pml_search_opts2 *opts, pml_result *out, pml_search_trace *traces /* n or NULL */);
void pml_search_trace_free(pml_search_trace *t);
/* host-only test door of the SPR candidate enumeration (the function the search itself calls): the prune cuts off the subtree
 * whose leaves are `pruned_leaves` (names joined by '\n'; a clade or a single leaf of the tree, else PML_ENOTFOUND); returned
 * are the regraft edges the engine would score for the window [rmin, rmax], in its order: distance_out[i] and, in *edges_out,
 * the leaf names on the far side of edge i joined by '\n', edges separated by an empty line.  An optional constraint matrix
 * (pml_search_opts' fields) removes the forbidden subtrees.  Release both arrays with pml_free. */
int pml_debug_spr_enumerate(const char *newick, const char *pruned_leaves, int rmin, int rmax, int nconstraints, int constraint_ntax,
                            const char *const *constraint_names, const char *const *constraint_rows, int *ncand_out,
                            int **distance_out, char **edges_out);
/* test door of the lazy SPR score (one gene, on the device): the same prune and window on the tree as given (lengths and
 * model->alpha as given, nothing optimised); lazy_out[i] = the score the search ranks candidate i by: the lnL of the tree with
 * the subtree regrafted into edge i, the joined branch tx + ty, the split edge halved, the pendant branch kept.
 * thorough_top != 0 (< 0 = all): the candidates with the best lazy scores also get the thorough insertion of pml_search2:
 * thorough_out[4 i ..] = its score, the pendant length, the near (towards the pruning point) and the far half of the split
 * edge it settled on -- the score is the lnL of the lazy tree with these three lengths; NaN for the other candidates. */
int pml_debug_spr_scores(pml_ctx *ctx, const pml_alignment *aln, const char *newick, const pml_model *model, const char *pruned_leaves,
                         int rmin, int rmax, int thorough_top, int *ncand_out, int **distance_out, char **edges_out, double **lazy_out,
                         double **thorough_out /* NULL ok when thorough_top == 0 */);

/* Models beyond WAG.  A rate matrix is 190 exchangeabilities -- the lower triangle by rows, (1,0), (2,0), (2,1), (3,0) ... in
 * the state order ARNDCQEGHILKMFPSTWYV -- and 20 frequencies: the layout of PAML's .dat files.
 * pml_matrix_parse_paml (host only) reads such a file's text; whatever follows the 210th number is ignored; fewer numbers, a
 * negative or a non-finite one: PML_EPARSE.
 * pml_matrix_register stores a matrix on the context and returns its model code (see PML_PI_REGISTERED); the frequencies
 * are normalised to sum 1.  Registering a name again replaces nothing, it returns a new code.  Thread-safe like every
 * context call.  Codes are accepted wherever PML_PI_EMPIRICAL is; pml_jackknife takes the own-frequency codes only and
 * refuses "F" codes and PML_PI_GTR at entry (pml_jackknife2 takes them all).
 * pml_model_eval is the reference's -matrix_eval loop (PhylogenomicPipeline2.java:1390-1452, getTreeScore :1482-1500) as ONE
 * device batch: the tree is optimised (branch lengths, alpha if opts says so, rates where the code is PML_PI_GTR) under each
 * of the nmodels codes; out[i] is what pml_optimize returns under codes[i] (4 categories, start alpha 1), bit for bit;
 * *best_out (optional) = index of the highest lnL, the first one of equals. */
int pml_matrix_parse_paml(const char *text, double *exch190, double *pi20);
int pml_matrix_register(pml_ctx *ctx, const char *name, const double *exch190, const double *pi20, int *code_out);
int pml_model_eval(pml_ctx *ctx, const pml_alignment *aln, const char *newick, int nmodels, const int *codes,
                   const pml_search_opts *opts, pml_result *out, int *best_out);

/* resident batches: encode + upload once, then evaluate repeatedly with inputs in HBM */
int  pml_batch_create(pml_ctx *ctx, int n, const pml_alignment *alns, const char *const *newicks,
                      const pml_model *model, pml_batch **out);
void pml_batch_destroy(pml_batch *b);
int  pml_batch_size(const pml_batch *b);
int  pml_batch_npatterns(const pml_batch *b, int gene);
/* full post-order CLV pass + root evaluation for every gene (all CLVs recomputed) */
int  pml_batch_score(pml_batch *b, double *lnl_out /* n */);
/* the same pass with every CLV WRITTEN to HBM (a child its parent consumes next is still read from registers): the whole-tree
 * traversal a search runs after a topology or alpha change, where later partial traversals read the CLVs back; same lnL bits */
int  pml_batch_score_stored(pml_batch *b, double *lnl_out /* n */);
int  pml_batch_site_lnl(pml_batch *b, int gene, double *site_lnl /* nsites */);
int  pml_batch_set_alpha(pml_batch *b, int gene /* -1 = all */, double alpha);
/* the rate matrix of one gene (or of all: gene -1) of a resident batch.  set: any batch becomes a batch of per-gene models;
 * pi20 NULL keeps the gene's frequencies.  get: what the gene is scored with -- the estimates after an optimisation under
 * PML_PI_GTR, the counted frequencies of an "F" variant; frequencies sum to 1 */
int  pml_batch_set_matrix(pml_batch *b, int gene /* -1 = all */, const double *exch190, const double *pi20 /* NULL = keep */);
int  pml_batch_get_matrix(pml_batch *b, int gene, double *exch190_out, double *pi20_out);
int  pml_batch_optimize(pml_batch *b, const pml_search_opts *opts, double *lnl_out, double *alpha_out);
int  pml_batch_search(pml_batch *b, const pml_search_opts *opts, double *lnl_out, double *alpha_out);
int  pml_batch_newick(pml_batch *b, int gene, int digits, char **out /* free with pml_free */);
/* d lnL/dt, d2 lnL/dt2 for the branch above each gene's taxon 0 (test hook for the Newton kernel) */
int  pml_batch_root_derivs(pml_batch *b, double *lnl, double *d1, double *d2);
void pml_free(void *p);

/* tree utilities (host) */
int pml_rf_distance(const char *newick_a, const char *newick_b, int *rf_out);
/* main tree with, on every internal branch, the number of support trees containing its bipartition
 * as an integer node label `)87:0.1`; *out is freed with pml_free */
int pml_support_tree(const char *main_newick, int ntrees, const char *const *support_newicks, int digits, char **out);

/* gene-wise jackknife (the data-parallel loop of the reference, one call):
 *   full tree  = search on the concatenation of ALL genes (NNI + SPR radius spr_radius_full),
 *   supports   = `reps` searches (NJ + NNI), each on the concatenation of `subset_size` genes drawn
 *                without replacement (0 = ngenes/2, PhylogenomicPipeline2.java:1599-1617),
 *   result     = full tree whose internal branches carry the number of support trees containing them.
 * Genes may cover different taxon subsets: the concatenation uses the sorted union of taxon names
 * and pads absent genes with '?' (MSAConcatenator.java:118-120,164-170).  The reference draws the
 * subsets from an unseeded java.util.Random; here the draw is seeded (deterministic). */
typedef struct {
    int reps;                    /* support trees (PEPR default 100) */
    int subset_size;             /* genes per replicate; 0 = ngenes / 2 */
    unsigned long long seed;
    int spr_radius_full;         /* SPR radius for the full tree (0 = NNI only) */
    double epsilon;              /* search epsilon (0 = 1e-3) */
    /* multi-GPU: every rank passes the same genes/seed; this call searches only replicates r with
     * r % shard_world == shard_rank and the full tree only on shard_rank 0 (elsewhere main_out->newick is
     * NULL and carries no supports); the caller gathers the support trees and decorates with
     * pml_support_tree (pepr_amd/distributed.py: jackknife()).  0,0 or world <= 1 = everything here. */
    int shard_rank, shard_world;
} pml_jackknife_opts;
int pml_jackknife(pml_ctx *ctx, int ngenes, const pml_alignment *genes, const pml_model *model,
                  const pml_jackknife_opts *opts, pml_result *main_out /* newick carries the supports */,
                  char **support_newicks_out /* optional: reps lines, '\n'-separated; pml_free */);
/* The same loop with the model the pipeline chose and with the decorator's counts:
 *   models    every valid pi_mode for the full tree (full_model) and for the support trees (support_model, NULL = the full
 *             tree's): the shared codes, PML_PI_EMPIRICAL, PML_PI_GTR, registered codes and registered + 1.  `-matrix_eval`
 *             hands mlMatrix to the full tree (PhylogenomicPipeline2.java:855-858) and to every gene-subset tree (:1247,
 *             :1619-1620); with FastTree supports (the default, :335-338) those stay WAG while the full tree uses mlMatrix.
 *             A replicate exists only as a code matrix in HBM, so a per-gene code gets its frequencies from a histogram of
 *             that matrix counted on the device (k_codehist): PML_PI_EMPIRICAL decomposes WAG with them, registered + 1 goes
 *             through the model-build kernel, PML_PI_GTR starts from WAG with them and estimates its rates as in any batch.
 *   counts    support_rule, applied to the support trees AS RETURNED in support_newicks_out:
 *             PML_SUPPORT_EQUAL_TAXA  pml_jackknife's rule: a replicate that lacks a taxon of the full tree supports nothing
 *             PML_SUPPORT_DECORATOR   TreeSupportDecorator.addSupportValues (:86-163) on those strings: every node of every
 *                       support tree, as its text roots it (after unroot()), adds Bipartition(its leaves found among the main
 *                       tree's sorted taxa, main taxon count) -- complement over the MAIN taxa, smaller side by cardinality, on
 *                       a tie the side holding the lowest index (Bipartition.java:41-64) -- to a multiset; a main branch gets
 *                       the multiset count of its own bipartition.  What a Java caller gets from decorating the strings; it
 *                       depends on where a subset tree's text is rooted.
 *             PML_SUPPORT_RESTRICTED  a replicate with taxon set S supports the main split A|B if A&S and B&S hold at least
 *                       two taxa each and the replicate has the split A&S | B&S: independent of any rooting
 *             For replicates over the main tree's taxon set the three rules agree.
 * base has pml_jackknife's meaning (draw, sub-batching by free HBM, sharding).  With support_model NULL, rule 0 and a shared
 * code the call returns pml_jackknife's strings. */
enum { PML_SUPPORT_EQUAL_TAXA = 0, PML_SUPPORT_DECORATOR = 1, PML_SUPPORT_RESTRICTED = 2 };
typedef struct {
    pml_jackknife_opts base;
    const pml_model *support_model;   /* NULL = the full tree's model */
    int support_rule;                 /* PML_SUPPORT_* */
} pml_jackknife_opts2;
int pml_jackknife2(pml_ctx *ctx, int ngenes, const pml_alignment *genes, const pml_model *full_model,
                   const pml_jackknife_opts2 *opts, pml_result *main_out, char **support_newicks_out);
/* The same loop with PEPR's tree-building methods for both kinds of tree (`-full_tree_method`, `-support_tree_method`;
 * PhylogenomicPipeline2.java:856-863, :1246, :1619; PhylogeneticTreeBuilder.java:104-115,136-161): maximum-parsimony trees
 * (`raxmlHPC -y`) are built from the genes resident in HBM -- k_fitch_tips writes every replicate's Fitch tip vectors straight
 * from the genes' code matrices, no concatenated text and no replicate code matrix -- and searched in lock step by pml_parsimony's
 * stepwise addition + SPR.
 *   support_method  PML_TREE_ML: as pml_jackknife2.  PML_TREE_PARSIMONY: every support tree is the parsimony tree of its
 *             replicate over the replicate's sorted taxon union, returned topology only (what pml_parsimony prints);
 *             base2.support_model is not used; the supports are counted under base2.support_rule as ever.  The replicates go
 *             through in sub-batches sized by their Fitch pools against the HBM budget of the ML replicates; the results do
 *             not depend on the split.  PML_TREE_PARSIMONY_BL is refused (PML_EINVAL): nothing reads a support tree's lengths.
 *   full_method     PML_TREE_ML: as pml_jackknife2.  PML_TREE_PARSIMONY: the parsimony tree of all genes; main_out->newick is
 *             topology only with the counts as inner labels `)87`; lnl, alpha and tree_length are 0, npatterns and nsites those
 *             of the concatenation.  PML_TREE_PARSIMONY_BL (`-y`, then `-f e -t`): the same topology, then branch lengths and
 *             alpha optimised under full_model from lengths 0.1 as pml_optimize does, to base.epsilon (0 = 1e-3); newick, lnl,
 *             alpha and tree_length come from that pass; per-gene model codes work as for any replicate.
 *   seeds     of the stepwise addition, independent of sharding and sub-batching: the full tree (unsigned)base.seed, replicate r
 *             (its index in pml_jackknife_draw's list) (unsigned)(base.seed + 1 + r); a value of 0 would mean "input order" and
 *             is replaced by 0x9E3779B9.
 *   limits    a replicate whose taxon union has fewer than 3 taxa fails the call (PML_EPARSE, "replicate r: parsimony needs at
 *             least 3 taxa").  Method values outside the lists above are PML_EINVAL, refused before anything is uploaded.
 * opts NULL = pml_jackknife2 with opts NULL.  With both methods PML_TREE_ML the call returns pml_jackknife2's strings and numbers. */
enum { PML_TREE_ML = 0, PML_TREE_PARSIMONY = 1, PML_TREE_PARSIMONY_BL = 2 };
typedef struct {
    pml_jackknife_opts2 base2;
    int full_method;        /* PML_TREE_*: how the full tree is built */
    int support_method;     /* PML_TREE_ML or PML_TREE_PARSIMONY */
    int parsimony_radius;   /* pml_parsimony_opts.spr_radius of every parsimony tree of the call (RAxML: 20; 0 = stepwise addition only) */
    int pad;
} pml_jackknife_opts3;
int pml_jackknife3(pml_ctx *ctx, int ngenes, const pml_alignment *genes, const pml_model *full_model,
                   const pml_jackknife_opts3 *opts, pml_result *main_out, char **support_newicks_out,
                   long long *mp_lengths_out /* optional, 1 + reps: [0] full tree, [1 + r] replicate r by its index in the draw;
                                                -1 = not a parsimony tree, or not built on this rank */);
/* k_fitch_tips launches (one per sub-batch of parsimony replicates, one per parsimony full tree, one per pml_debug_fitch_tips) and
 * k_fitch launches (every device step of every parsimony tree, pml_parsimony* included) on this context so far.  Never reset. */
int pml_fitch_stats(pml_ctx *ctx, long long *tips_launches, long long *fitch_launches);
/* test door of k_fitch_tips, the counterpart of pml_debug_gather: encodes the genes into HBM, fills the Fitch tip vectors of the
 * selection `sel` (NULL = all) exactly as pml_jackknife3 does for a replicate and reads them back: masks_out[ntax x mpad] (bit s =
 * amino acid s possible; B = N|D, Z = Q|E, gap / unknown / absent taxon / padding = 0xFFFFF), weights_out[mpad] (0 = padding),
 * names_out = the sorted taxon union, one per line.  The three buffers are released with pml_free. */
int pml_debug_fitch_tips(pml_ctx *ctx, int ngenes, const pml_alignment *genes, int nsel, const int *sel, int *ntax_out,
                         int *npat_out, int *mpad_out, unsigned **masks_out, int **weights_out, char **names_out);
/* host-only: pml_support_tree under one of the PML_SUPPORT_* rules; support trees may cover other taxon sets than the main
 * tree's (rule 0 counts such a tree as not supporting, where pml_support_tree returns PML_EPARSE) */
int pml_support_tree_rule(const char *main_newick, int ntrees, const char *const *support_newicks, int rule, int digits,
                          char **out);
/* test hook for k_codehist, as pml_debug_gather is for k_gather: gathers the selection `sel` (NULL = all genes) on the device
 * in one batch with the replicate of all genes, counts both code matrices in one launch and reads the selection's result
 * back: counts_out[code] = the number of cells (taxon x site, absent taxa = gap cells) holding the code, pi_out = the
 * empirical frequencies of the "F" scheme from those counts */
int pml_debug_replicate_freqs(pml_ctx *ctx, int ngenes, const pml_alignment *genes, int nsel, const int *sel,
                              long long counts_out[23], double pi_out[20]);
/* host-only: the gene subsets pml_jackknife draws for (ngenes, reps, subset_size, seed) -- replicate r = sel_out[r*k .. r*k+k),
 * ascending gene indices, k = the return value (subset_size, or ngenes/2 when 0; < 0 = error).  The reference draws them with
 * RandomSetUtils.getRandomSet (.../pepr/util/RandomSetUtils.java:9-35, unseeded java.util.Random); callers that need to know
 * which genes a support tree was built from (reports, the oracle-side parity test) get the seeded draw here. */
int pml_jackknife_draw(int ngenes, int reps, int subset_size, unsigned long long seed, int *sel_out /* reps x k */);
/* test hook for the device-side concatenation (MSAConcatenator.java:78-189): encodes the genes into HBM, gathers
 * the selection `sel` (NULL = all) on the device exactly as pml_jackknife does for a replicate, and reads the result back:
 * codes_out[ntax x mpad] (0..19 = ARNDCQEGHILKMFPSTWYV, 20 = B, 21 = Z, 22 = gap/unknown), weights_out[mpad] (0 = padding),
 * names_out = the sorted taxon union, one per line.  The three buffers are released with pml_free. */
int pml_debug_gather(pml_ctx *ctx, int ngenes, const pml_alignment *genes, int nsel, const int *sel, int *ntax_out,
                     int *npat_out, int *mpad_out, unsigned char **codes_out, double **weights_out, char **names_out);
/* test door of the model-build kernel (k_model): the eigen-systems of n rate matrices (n x 190 exchangeabilities, n x 20
 * frequencies) as the device structs, sizeof(ModelDev) / 8 = 1240 doubles each: eval[20], U[20][20] (P(t) = U diag(exp(eval t))
 * Uinv), Uinv[20][20], pi[20], Uinv transposed [20][20] */
int pml_debug_model_build(pml_ctx *ctx, int n, const double *exch /* n x 190 */, const double *pi /* n x 20 */,
                          double *modeldev_out /* n x 1240 */);
/* host-only: the refinement loop's support queries on a rooted Newick with support labels (")95:0.1" or
 * ":0.1[95]"; missing = 100, fractions are x100) -- PhylogeneticTreeRefiner.java:298-359 getNextIndexToRefine,
 * AdvancedTree.java:1061-1098 getMeanDescendantSupportValues.  *ingroup_out = comma-joined sorted leaf names of
 * the next clade to refine, NULL if none; done[] = clades already refined in the same format (the caller's
 * refinedSubsets).  mean_out (optional) = floor(mean descendant support) per node in order of appearance. */
int pml_refine_next(const char *supported_newick, int cutoff, int ndone, const char *const *done,
                    char **ingroup_out, int *nnodes_out, int **mean_out /* pml_free */);
/* SH-like local supports, FastTree's default output when -nosupport is absent (FastTreeRunner.java:67-70: PEPR drops
 * -nosupport when bootstrapReps > 0; AdvancedTree.getBranchSupports :484-506 reads the 0-1 labels x100).  For every
 * internal split of the given tree (lengths and model->alpha as given): the split's arrangement against its two NNI
 * alternatives, `nboot` (FastTree: 1000) resamples of the alignment columns on the device, support = share of
 * resamples that do not overturn the observed advantage (FastTree 2.1 SHSupport / Guindon et al. 2010).
 * out[i].newick carries the supports as inner labels with 3 decimals; lnl = lnL of the tree. */
int pml_sh_support(pml_ctx *ctx, const pml_alignment *aln, const char *newick, const pml_model *model,
                   int nboot, unsigned long long seed, pml_result *out);
int pml_sh_support_batch(pml_ctx *ctx, int n, const pml_alignment *alns, const char *const *newicks,
                         const pml_model *model, int nboot, unsigned long long seed, pml_result *out);
/* FastTree's `-gamma` likelihood (FastTreeRunner.java:67-70 passes -gamma on every call; SURVEY 8a-11 vi): the given tree's
 * per-site likelihoods at FastTree's 20 fixed rates 0.05 * 400^(k/19) (five device traversals of four rates), re-weighted
 * by a discretised Gamma(alpha) with mean `rescale`; alpha and rescale are fitted on that table.  out[i].lnl = Gamma20 lnL,
 * out[i].alpha = its alpha, out[i].newick = the tree with every length multiplied by rescale_out[i] (what FastTree prints),
 * out[i].tree_length of that tree.  model->pi_mode selects the frequencies (FastTree_WAG: PML_PI_WAG_FULL); model->alpha
 * and ncat are not used. */
int pml_gamma20(pml_ctx *ctx, const pml_alignment *aln, const char *newick, const pml_model *model, pml_result *out,
                double *rescale_out);
int pml_gamma20_batch(pml_ctx *ctx, int n, const pml_alignment *alns, const char *const *newicks, const pml_model *model,
                      pml_result *out, double *rescale_out /* n, may be NULL */);
/* Maximum-parsimony trees (Fitch lengths on the device): randomised stepwise addition (seed 0 =
 * input order) then SPR hill climbing within spr_radius edges (0 = none; RAxML uses 20).  out[i].newick is
 * topology only; out[i].lnl / alpha / tree_length are 0; mp_length[i] (optional) = weighted Fitch length. */
typedef struct { unsigned seed; int spr_radius; } pml_parsimony_opts;
int pml_parsimony(pml_ctx *ctx, const pml_alignment *aln, const pml_parsimony_opts *opts, pml_result *out, long long *mp_length);
int pml_parsimony_batch(pml_ctx *ctx, int n, const pml_alignment *alns, const pml_parsimony_opts *opts,
                        pml_result *out, long long *mp_length);
/* Non-parametric bootstrap (`raxmlHPC -f a -x seed -N reps`, RAxMLRunner.java:115-132): best ML tree (NNI + SPR)
 * labelled with the percentage of `reps` column-resampled replicate trees (one device batch) containing each
 * bipartition, as RAxML_bipartitions.<run> carries them (read at RAxMLRunner.java:302-318). */
int pml_bootstrap(pml_ctx *ctx, const pml_alignment *aln, const pml_model *model, int reps, unsigned long long seed,
                  int spr_radius_best, double epsilon, pml_result *best_out,
                  char **replicate_newicks_out /* optional: reps lines; pml_free */);
/* The column bootstrap of a gene set as a resident call: `raxmlHPC -f a -x seed -N reps` (PML_TREE_ML) and `-Y -N reps`
 * (PML_TREE_PARSIMONY, PML_TREE_PARSIMONY_BL) on the concatenation of `genes` (taxa = sorted union, a gene that lacks a taxon
 * contributes gaps), the path PhylogenomicPipeline2.buildConcatenatedTree (:836-890) takes with bootstrapReps through
 * PhylogeneticTreeBuilder.java:136-181.  The genes are encoded once into HBM; no resampled text is built.
 *   column space   the genes in the order given: L = sum of nsites columns, P = sum of npat patterns (compressed per gene, never
 *             across genes); column c of gene g with local site s has pattern id off_g + site2pat_g[s].
 *   draws     replicate r has the key K_r = mix64((seed + 1) * 0x9E3779B97F4A7C15 + r), mix64 = splitmix64's finaliser; draw j
 *             (0 <= j < L) is column c_j = ((mix64(K_r + j) >> 32) * L) >> 32, the multiply-shift rule of pml_step_thresholds.
 *             count[r][p] = the draws that land on pattern p (sum = L); replicate r is the patterns with count > 0 in ascending
 *             p, each with weight count[r][p], padded to a multiple of 32 patterns with weightless gaps.  The draws are the
 *             project's own (RAxML's -x stream lives inside its binary): parity unpinned, as for pml_step_thresholds.
 *   best tree      PML_TREE_ML: NNI + SPR within spr_radius_best on the replicate of all genes, as pml_jackknife* builds its full
 *             tree.  PML_TREE_PARSIMONY: the parsimony tree of all genes, topology only; lnl, alpha, tree_length 0.
 *             PML_TREE_PARSIMONY_BL: that topology, then lengths and alpha optimised under `model` (`-f e`).
 *   replicates     PML_TREE_ML: the NNI search from the neighbour-joining tree of the replicate's weighted pair counts, under
 *             replicate_model.  Parsimony (both methods): parsimony trees within parsimony_radius, returned topology only --
 *             nothing reads their lengths.  Stepwise-addition seeds: the best tree (unsigned)seed, replicate r (unsigned)(seed +
 *             1 + r), 0 replaced by 0x9E3779B9, as pml_jackknife3.  The replicates go through in sub-batches sized against free
 *             HBM; the result does not depend on the split.
 *   labels    best_out->newick carries (int)(0.5 + 100 c / reps) per bipartition, c = the replicate trees that contain it, as
 *             pml_bootstrap; with reps == 0 it carries no labels.  npatterns = P, nsites = L.
 * RAxML's rapid-bootstrap shortcuts (CAT approximation, tree reuse between replicates) and whatever files `-Y -N` writes are not
 * restated: every replicate gets a search of its own.  PML_EINVAL with a message: reps < 0, an unknown method, fewer than 3 taxa
 * in the union, L < 1 or L >= 2^31.  opts NULL = 100 ML replicates, seed 0, radius 5 / 20. */
typedef struct {
    int reps; int method;              /* PML_TREE_ML | PML_TREE_PARSIMONY | PML_TREE_PARSIMONY_BL */
    unsigned long long seed;
    int spr_radius_best;               /* ML best tree, as pml_bootstrap */
    int parsimony_radius;              /* as pml_jackknife_opts3 */
    double epsilon;                    /* 0 = 1e-3 */
    const pml_model *replicate_model;  /* NULL = model; any code pml_jackknife2 accepts */
} pml_bootstrap_opts2;
int pml_bootstrap2(pml_ctx *ctx, int ngenes, const pml_alignment *genes, const pml_model *model, const pml_bootstrap_opts2 *opts,
                   pml_result *best_out, char **replicate_newicks_out /* optional: reps lines; pml_free */,
                   long long *mp_lengths_out /* optional, 1 + reps: [0] best tree, [1 + r] replicate r; -1 = not a parsimony tree */);
/* the log likelihoods the ML replicates of the last pml_bootstrap2 call on this context ended their searches with, in replicate
 * order (their Newick lines carry none): writes min(n, count) values, returns the count.  The values are state of the context:
 * every pml_bootstrap2 call clears them on entry, so the count is 0 after a parsimony call, a refused call, or none; after a call
 * that failed part-way it counts the sub-batches that finished */
int pml_boot_replicate_lnls(pml_ctx *ctx, int n, double *lnl_out);
/* host-only, no context: the ncols columns replicate `rep` of a call with `seed` draws, in draw order, from the functions the
 * kernel runs (csrc/boot.hpp).  PML_EINVAL: rep < 0, ncols < 1 or ncols >= 2^31 */
int pml_boot_draws_host(unsigned long long seed, int rep, long long ncols, unsigned *cols_out);
/* the patterns k_boot_index compacts per step of its scan */
int pml_boot_tile(void);
/* test door: what the device builds for replicate `rep` of the selection `sel` (NULL = all genes), read back.  idx_out[npat] = the
 * replicate's pattern ids, ascending; form 0: cells_out = the code matrix uint8 [ntax x mpad] (padding = the gap code 22),
 * weights_out = f64 [mpad] (padding 0), as an ML batch holds them; form 1: cells_out = the Fitch state sets uint32 [ntax x mpad]
 * (padding 0xFFFFF), weights_out = int [mpad], as a parsimony pool holds them (mpad >= 32); cmp_out / diff_out [ntax x ntax] = the
 * weighted comparable / differing column counts of every taxon pair (k_boot_pairs; from the form 0 build in both forms, so form 1
 * runs count, index and gather twice).  names_out: one taxon per line.  Everything returned is freed with pml_free. */
int pml_debug_boot_replicate(pml_ctx *ctx, int ngenes, const pml_alignment *genes, int nsel, const int *sel, unsigned long long seed,
                             int rep, int form, int *ntax_out, int *npat_out, int *mpad_out, int **idx_out, void **cells_out,
                             void **weights_out, long long **cmp_out, long long **diff_out, char **names_out);
/* launches on this context so far: [0] k_boot_count, [1] k_boot_index, [2] k_boot_gather, [3] k_boot_pairs; with cfg.profile = 1
 * kernel_ms holds their summed HIP-event times; build_ms = the host wall time of the replicate builds (count, index, layout,
 * gather, pair counts and NJ starts, or the tip rows of a pool).  Any pointer may be NULL.  Never reset. */
int pml_boot_stats(pml_ctx *ctx, long long *launches /* [4] */, double *kernel_ms /* [4] */, double *build_ms);
/* host-only: FASTA text (">taxon\nSEQ\n" per taxon, SequenceAlignment.java:405-416) of the
 * concatenation of the selected genes (sel == NULL: all), taxa = sorted union, '?' padding */
int pml_concatenate(int ngenes, const pml_alignment *genes, int nsel, const int *sel, char **fasta_out);

/* Tree selection tests (TreeComparison.java:812-885: makermt -b 10 --puzzle | consel | catpv -v): which of T candidate trees
 * do the data reject?  Multiscale RELL bootstrap on the device: K scales r_k, at scale k every one of B replicates draws
 * n_k = max(1, floor(r_k N + 0.5)) sites with replacement and sums their per-site lnL for every tree.
 *   draws    site_j = ((mix64(base + ((k B + b) << 32) + j) >> 32) * N) >> 32 for draw j of replicate b at scale k, with
 *            base = (seed + 1) * 0x9E3779B97F4A7C15 mod 2^64 and mix64 the finaliser of splitmix64; a site is drawn with
 *            probability within 2^-32 of 1 / N (a relative non-uniformity of at most N / 2^32).  N < 2^31, K B < 2^32, 2 <= T <= 64.
 *   sums     Y[k][b][t] = sum_j lnl[t][site_j], plain double additions in ascending j: a function of (seed, k, b, N, table)
 *            alone, the same bits whatever else the call holds and whichever device path (LDS or global memory) serves it
 *   counts   bp[k][t]: replicates of scale k whose best tree is t (the lowest index of equals), every scale.  At the scale
 *            k1 whose n_k / N is closest to 1 (the first of equals), with L_t = sum_s lnl[t][s] in site order and
 *            C_t = Y_t (N / n_k) - L_t:   sh[t]: max_u C_u - C_t >= max_u L_u - L_t;   kh[t]: C_u* - C_t >= L_u* - L_t with
 *            u* = argmax_{u != t} L_u (the lowest index of equals).  The replicates are centred on their exact expectation
 *            L_t, where CONSEL centres on the replicate mean (a second pass); the two differ by O(B^-1/2) of a replicate's spread.
 *   p-values kh, sh, bp = np = counts / B at scale k1 (Kishino-Hasegawa 1989, Shimodaira-Hasegawa 1999); au = the approximately
 *            unbiased test of Shimodaira 2002 fitted to the K bootstrap counts of the tree (pml_au_fit); pp = exp(L_t - max) / sum.
 *            consel's maximum-likelihood fit and its model selection are not built.  No CONSEL
 *            binary or source is part of the reference, so parity with CONSEL's own output is NOT pinned: the definitions are
 *            the published ones, and the tests check them against an independent restatement.
 *   weighted (the *_weighted calls; catpv's last two columns)  For a pair of trees d_s = lnl[u][s] - lnl[t][s], mean = (sum_s d_s) / N,
 *            sigma_ut^2 = N / (N - 1) sum_s (d_s - mean)^2: the variance of the difference of the totals (Kishino-Hasegawa 1989),
 *            summed over the centred differences in two passes on the device (never from a Gram matrix sum x_u x_t, which
 *            cancels about five digits at per-site lnL near -40).  sigma_ut = 0 (N = 1, or two identical columns) excludes
 *            the pair from every weighted statistic of both trees; a tree with no pair left gets wkh = wsh = 1 and counts
 *            equal to B.  At scale k1, over the very replicates of kh / sh:
 *              wsh[t]: S*_t >= S_t with S_t = max_u (L_u - L_t) / sigma_ut and S*_t = max_u (C_u - C_t) / sigma_ut
 *                      (Shimodaira-Hasegawa 1999, weighted form), u != t with sigma_ut > 0;
 *              wkh[t]: (C_u* - C_t) / sigma_u*t >= (L_u* - L_t) / sigma_u*t with u* = argmax_u (L_u - L_t) / sigma_ut, the lowest
 *                      index of equals.  For a fixed u* the sigma cancels: wkh differs from kh only through the choice of u*
 *                      (the most significant competitor instead of the one with the highest lnL).
 *            Every division is a multiplication by the precomputed 1 / sigma_ut: one rounded multiply of a rounded difference.
 *            CONSEL estimates the variance from its replicates; here it is the exact site variance, for the reason the
 *            replicates are centred on L_t and not on their mean: one pass less, and the two differ by O(B^-1/2).
 * Every array of pml_tree_test_result is allocated by the library; release with pml_tree_test_result_free. */
typedef struct {
    int nscales;                 /* 0 = 10 */
    const double *scales;        /* nscales values r_k > 0; NULL = 0.5, 0.6 ... 1.4 (nscales 0 or 10) */
    long long reps_per_scale;    /* B; 0 = 10 000; PEPR's `makermt -b 10` = 100 000 */
    unsigned long long seed;
} pml_tree_test_opts;
typedef struct {
    int ntrees, nscales, k1;     /* k1: the scale of np / bp / kh / sh */
    long long nsites, reps;
    double *scales;              /* [nscales] n_k / N as drawn */
    long long *ndraws;           /* [nscales] n_k */
    double *lnl;                 /* [ntrees] pml_rell_tests: L_t; pml_tree_tests: the engine's lnL of the tree (the bits of pml_optimize) */
    double *obs;                 /* max_{u != t} L_u - L_t */
    double *au, *np, *bp, *kh, *sh, *pp;
    double *au_d, *au_c, *au_rss; int *au_nused;     /* the AU fit: signed distance, curvature, weighted residual sum, scales used */
    int *rank;                   /* 1 = highest L_t; equals in index order */
    long long *bp_count;         /* [nscales][ntrees] */
    long long *kh_count, *sh_count;   /* [ntrees] */
} pml_tree_test_result;
/* host-only (no device needed): Shimodaira's weighted least squares.  Over the scales with 0 < count_k < B:
 * z_k = -Phi^-1(count_k / B) (Phi^-1 by algorithm AS 241, PPND16), weights B phi(z_k)^2 / (p_k (1 - p_k)), fit
 * z_k ~ d sqrt(r_k) + c / sqrt(r_k); *au = 1 - Phi(d - c), *rss = the weighted residual sum of squares.  Fewer than two usable
 * scales, or usable scales that do not determine d and c (normal matrix singular to 1e-12 of its diagonal product: all of one
 * r_k): *au = count[k1] / B, d = c = rss = 0 and *nused = 0 or 1 -- *nused >= 2 always means that the curve was fitted.
 * d, c, rss, nused may be NULL. */
int pml_au_fit(int nscales, const double *r /* n_k / N */, const long long *count, long long B, double *au, double *d, double *c,
               double *rss, int *nused);
/* site_lnl: ntrees rows of nsites per-site lnL, the layout of RAxML_perSiteLLs */
int pml_rell_tests(pml_ctx *ctx, long long nsites, int ntrees, const double *site_lnl, const pml_tree_test_opts *opts,
                   pml_tree_test_result *out);
/* The whole chain: the ntrees trees are ONE device batch; search_opts != NULL optimises every tree's branch lengths (and alpha if
 * optimize_alpha) to search_opts->epsilon (0 = 1e-4) as `raxmlHPC -f g` does before it writes per-site lnL -- nni, spr_radius,
 * seed and constraints are not used -- and NULL scores the trees as given.  The table is built on the device from the
 * per-pattern lnL of that batch.  site_lnl_out (optional, ntrees x nsites) receives the very values that were resampled. */
int pml_tree_tests(pml_ctx *ctx, const pml_alignment *aln, int ntrees, const char *const *newicks, const pml_model *model,
                   const pml_search_opts *search_opts, const pml_tree_test_opts *test_opts, pml_tree_test_result *out,
                   double *site_lnl_out);
void pml_tree_test_result_free(pml_tree_test_result *r);
/* test door of the resampling kernel (k_rell): scale k draws ndraws[k] sites; y_out (optional, small shapes) = every replicate
 * sum Y[nscales][reps][ntrees]; the raw counts bp_out[nscales][ntrees], kh_out / sh_out[ntrees].  path: 0 = LDS when the table
 * fits, 1 = LDS (PML_EINVAL when it does not fit), 2 = global memory; *path_used = 1 or 2.  kernel_ms_out (optional): HIP-event
 * time of the resampling launch. */
int pml_debug_rell(pml_ctx *ctx, long long nsites, int ntrees, const double *site_lnl, int nscales, const long long *ndraws,
                   long long reps, unsigned long long seed, int path, double *y_out, long long *bp_out, long long *kh_out,
                   long long *sh_out, int *path_used, double *kernel_ms_out);

/* The weighted columns of the same replicates (definitions above).  Arrays are allocated by the library; release with
 * pml_tree_test_weighted_free. */
typedef struct {
    int ntrees;
    double *wkh, *wsh;                  /* [ntrees] counts / B */
    long long *wkh_count, *wsh_count;   /* [ntrees] */
    double *sigma;                      /* [ntrees][ntrees] sigma_ut, 0 on the diagonal and for excluded pairs */
    int *wkh_other;                     /* [ntrees] u*, -1 if the tree has no pair */
} pml_tree_test_weighted;
/* pml_rell_tests / pml_tree_tests with the weighted columns: `out` receives exactly what the unweighted call returns for the
 * same arguments, bit for bit; `wout` the weighted columns counted over the same replicates in the same launch. */
int pml_rell_tests_weighted(pml_ctx *ctx, long long nsites, int ntrees, const double *site_lnl, const pml_tree_test_opts *opts,
                            pml_tree_test_result *out, pml_tree_test_weighted *wout);
int pml_tree_tests_weighted(pml_ctx *ctx, const pml_alignment *aln, int ntrees, const char *const *newicks, const pml_model *model,
                            const pml_search_opts *search_opts, const pml_tree_test_opts *test_opts, pml_tree_test_result *out,
                            pml_tree_test_weighted *wout, double *site_lnl_out);
void pml_tree_test_weighted_free(pml_tree_test_weighted *w);
/* test door of the weighted arm of k_rell and of k_rell_pairsd: pml_debug_rell's arguments and results (the same bits), plus
 * inv_sigma_in ([ntrees][ntrees] 1 / sigma_ut: symmetric, >= 0, 0 on the diagonal, 0 = pair excluded; NULL = computed by
 * k_rell_pairsd), inv_sigma_out (optional, the matrix that was used) and the raw counts wkh_out / wsh_out[ntrees].  The LDS path
 * needs room for the table plus the matrix. */
int pml_debug_rell_weighted(pml_ctx *ctx, long long nsites, int ntrees, const double *site_lnl, int nscales, const long long *ndraws,
                            long long reps, unsigned long long seed, int path, double *y_out, long long *bp_out, long long *kh_out,
                            long long *sh_out, int *path_used, double *kernel_ms_out, const double *inv_sigma_in,
                            double *inv_sigma_out, long long *wkh_out, long long *wsh_out);
/* host-only: the table as runConsel's caller receives it from `catpv -v`, lines joined by '\n' (release with pml_free): a header
 * line and one line per tree in rank order (equal ranks in index order):
 *   "# rank item      obs     au     np |     bp     pp     kh     sh    wkh    wsh |"
 *   "# %4d %4d %8.1f %6.3f %6.3f | %6.3f %6.3f %6.3f %6.3f %6.3f %6.3f |"      item = 1-based index of the tree
 * w == NULL prints "-" right-aligned in the two weighted columns.  No catpv binary or source is part of the reference: the
 * columns and their order are catpv's documented ones, the exact spacing is this project's definition. */
int pml_catpv_table(const pml_tree_test_result *r, const pml_tree_test_weighted *w, char **out);

/* The reference's `nj` tree-building method (PhylogeneticTreeBuilder.java:198-208, PhylogenomicPipeline2.java:1279-1293), the one
 * method whose reference is source code: parity is PINNED here -- same topology and child order in the text, every branch length
 * the same bits as the Java's double (the spelling of the numbers is this library's: the shortest of 15, 16 or 17 significant
 * digits that reads back to the same double, so "0" where Java prints "0.0").
 *   codes   ARNDCQEGHILKMFPSTWYV = 0..19, B = 20, Z = 21, X = 22, '-' and '?' = 23, either letter case
 *           (AlignmentUtilities.convertAminaAcidSequenceToInts :174-342).  The Java DROPS every other byte (J, O, U, *, '.', digits,
 *           blanks) and shifts the rest of the row; that is not reproduced: such an alignment is refused with PML_EPARSE, and
 *           pml_last_error names the taxon, the column (0-based) and the byte.
 *   table   24 x 24 ints, row major, table[c_i][c_j], entries in [-128, 127] (else PML_EINVAL).  NULL = BLOSUM62 as
 *           loadScoringMatrixFromResource (:371-398) leaves it (pml_pairscore_table_blosum62): rows and columns 0..22 are the first
 *           23 of the file, whose order is A..V B J Z X *, so code Z reads the file's J line, code X the file's Z line, and the gap
 *           row and column are 0.  A table need not be symmetric: every ordered pair is computed.
 *           A taxon that a gene of a concatenation lacks is a row of '?': it scores table[gap][c] against code c, whatever the table.
 *   scores  S[i][j] = -1 + sum_k table[c_i(k)][c_j(k)] (SequenceAlignment.getPairwiseScores :1042-1067; the -1 is its
 *           Arrays.fill), diagonal included, computed on the device (k_pairscore); exact integers.
 *   trees   PML_NJ_TREE = TreeBuilder.getNJTreeString (:152-344): similarities become distances max(0, max_i S[i][i]) - S (non-zero
 *           diagonal, row sums include it), Q = (n-2) D - sum_i - sum_j, the first strict minimum over i < j in row-major order is
 *           merged, its two lengths are clamped at 0, the merged node goes to index 0; the last three lengths are NOT clamped
 *           (negative lengths are printed).  PML_NJ_TOPOLOGY = getNJTopology (:34-140), the `-nj true` path: the first strict
 *           maximum of the similarities (minimum of distances) is merged, new values are plain means, "(x,y);" without lengths.
 *           Fewer than 4 taxa: PML_EINVAL (the Java returns null for 3).
 * The score of a concatenation is the sum of its genes' scores (a taxon a gene lacks is a row of '?': 0), so the calls that take
 * genes compute every gene's matrix once, in one k_pairscore launch (more when the code bytes are uploaded in sub-batches by free
 * HBM; PML_HBM_BUDGET_MB as for pml_jackknife), and build each replicate's matrix as an integer sum on the device. */
enum { PML_NJ_DISTANCE = 0, PML_NJ_SIMILARITY = 1 };
enum { PML_NJ_TREE = 0 /* getNJTreeString */, PML_NJ_TOPOLOGY = 1 /* getNJTopology */ };
int pml_pairscore_table_blosum62(int table_out[576]);                                  /* host-only */
/* host-only: the tree of an n x n matrix (row major) of the given type; *newick_out is released with pml_free */
int pml_nj_from_matrix(int n, const char *const *names, const double *m, int matrix_type, int form, char **newick_out);
int pml_pairwise_scores(pml_ctx *ctx, const pml_alignment *aln, const int *table576 /* NULL = BLOSUM62 as loaded */,
                        double *scores_out /* ntax*ntax */);
/* buildNeighborJoiningTree (form PML_NJ_TREE) / buildConcatenatedNeighborJoiningTree (PML_NJ_TOPOLOGY) of one alignment */
int pml_nj_tree(pml_ctx *ctx, const pml_alignment *aln, const int *table576, int form, char **newick_out);
/* nrep trees, replicate r = the concatenation (MSAConcatenator: sorted taxon union) of the genes sel[r*k .. r*k+k); sel NULL with
 * nrep 1 = all genes.  newicks_out: nrep lines; scores_out (optional): the replicates' nu x nu score blocks one after the other;
 * ntax_out (optional): nu per replicate.  All three are released with pml_free. */
int pml_nj_replicates(pml_ctx *ctx, int ngenes, const pml_alignment *genes, int nrep, int k, const int *sel, const int *table576, int form,
                      char **newicks_out, double **scores_out, int **ntax_out);
/* The gene-wise jackknife with NJ trees throughout: the full tree (getNJTreeString on all genes) and opts->reps support trees on
 * the subsets pml_jackknife_draw gives for (ngenes, reps, subset_size, seed), ONE k_pairscore launch for all of it; the supports
 * are counted on the returned strings under support_rule (PML_SUPPORT_*) and written behind the ')' of the main tree's inner
 * nodes, whose text and lengths are otherwise the NJ tree's own.  shard_world > 1 is refused (PML_EINVAL): the whole loop is
 * cheaper than a gather.  spr_radius_full and epsilon are not used. */
int pml_nj_jackknife(pml_ctx *ctx, int ngenes, const pml_alignment *genes, const pml_jackknife_opts *opts, const int *table576,
                     int support_rule, char **main_newick_out, char **support_newicks_out);
/* test hook of k_pairscore: the raw sums (without the -1) with chunk_sites sites per workgroup (a multiple of 16, at most 2^20;
 * 0 = the default), so that small alignments cross chunk boundaries */
int pml_debug_pairscores(pml_ctx *ctx, const pml_alignment *aln, const int *table576, int chunk_sites, long long *out /* ntax*ntax */);
/* k_pairscore_sum launches on this context so far (one per pml_nj_replicates / pml_nj_jackknife call) and, with cfg.profile = 1,
 * their summed HIP-event time; k_pairscore itself is counted by pml_kernel_stats(PML_K_PAIRSCORE).  Never reset. */
int pml_pairscore_sum_stats(pml_ctx *ctx, long long *launches, double *total_ms);

/* The reference's `-congruence_filter` (HandyConstants.java:86, PhylogenomicPipeline2.java:234-247, filterForCongruence :429-511):
 * which genes enter the concatenation, decided before any tree is built.  The taxa are the sorted union of the genes' names
 * (n of them, at most 512; taxon i = bit i & 63 of word i >> 6 of a split's W = 1, 2, 4 or 8 64-bit words).  Bytes are compared
 * by identity (no alphabet: 'a' and 'A' differ); only '-' and '?' are special; a taxon a gene lacks reads '?' in its columns.
 *   splits   of a column (SequenceAlignment.getBipartitionsForAlignmentColumn :808-882): none when every byte is '-' or '?';
 *            else, for every other distinct byte, the set of taxa that show it, normalised (Bipartition.java:41-64): complement
 *            over ALL n taxa, the side with fewer members kept, on a tie the side that holds taxon 0.  Two classes that cover all
 *            n taxa are one split.  A class of all taxa is the empty split.
 *   counts   count(s) = the columns, over all genes, that have split s, for every s of at least 2 members (getBipartitionsForColumns
 *            :697-719).  Counted per distinct split: the Java's Arrays.sort on a hash difference is a grouping device whose int
 *            can overflow from 32 taxa upward, and then loses counts depending on the JDK's sort; below 32 taxa the two agree.
 *   kept     (BipartitionSet.setBipartitions :84-139) with dist[c] = the number of distinct splits of count c: cutoff steps down
 *            from the largest count while fewer than 4 n splits are included; K = every split with count >= cutoff, ties
 *            included, so |K| has no bound.
 *   cost     of a split b (getCost :642-652, isCompatible Bipartition.java:125-149) = the sum of count(k) over the k in K with
 *            b & k non-empty, != b and != k.
 *   genes    cost_sum = the sum of the costs of the gene's DISTINCT splits (trivial ones included, each once), summed in 64 bits
 *            (the Java's int wherever that does not overflow); mean_cost = cost_sum / columns by integer division.  A gene
 *            without columns is PML_EPARSE (the Java drops it from one of two arrays that it indexes with one counter).
 *   select   p = trim_percent, divided by 100 when >= 1.0 (:191-195); idx = (int)(G - G p) in doubles; max_cost = the idx-th of
 *            the ascending mean costs; gene g is kept iff g <= idx and mean_cost[g] <= max_cost (:497).  The first condition
 *            compares the gene's POSITION in the input with a rank: that is the Java as it stands (with 20 genes and p = 0.1
 *            gene 19 always goes).  p <= 0, NaN, or an idx outside the genes: PML_EINVAL (the Java throws).
 * Splits are extracted, interned, counted and charged on the device (congruence.hip); K is chosen on the host.  The whole call
 * is resident: when its records do not fit the HBM budget (0.85 of free HBM, or PML_HBM_BUDGET_MB) it is refused with PML_ENOMEM
 * and a message that gives the size. */
typedef struct {
    int use_hash_mask;                /* test door: 0 = production (all ones) */
    unsigned long long hash_mask;     /* ANDed onto every hash value before it is reduced to a slot: 0 makes every key probe from slot 0 */
} pml_congruence_opts;
typedef struct {
    int ngenes, ntax, words;          /* G, n, W */
    char **names;                     /* n sorted taxon names */
    long long *cost_sum, *mean_cost;  /* [G] */
    int *nsplits;                     /* [G] distinct splits of the gene, trivial ones included */
    int cutoff;
    long long nkept;                  /* |K| */
    unsigned long long *kept_words;   /* [|K|][W], ascending as n-bit integers (word W-1 most significant) */
    long long *kept_count, *kept_cost;/* [|K|]: what BipartitionSet.printBipartitionsAndCounts lists, and each kept split's own cost */
    long long nrecords, ndistinct;    /* split records of all columns; distinct splits among them */
} pml_congruence_result;
int  pml_congruence_costs(pml_ctx *ctx, int ngenes, const pml_alignment *genes, const pml_congruence_opts *opts /* NULL = production */,
                          pml_congruence_result *result);
void pml_congruence_result_free(pml_congruence_result *result);
/* host-only: the selection rule; keep_out[G] = 1 / 0; idx_out and max_cost_out are optional */
int  pml_congruence_select(int ngenes, const long long *mean_cost, double trim_percent, int *keep_out, int *idx_out, long long *max_cost_out);
int  pml_congruence_filter(pml_ctx *ctx, int ngenes, const pml_alignment *genes, double trim_percent, int *keep_out,
                           pml_congruence_result *result /* may be NULL */);
/* test hook of k_colsplits: the split records of one gene's columns over the given sorted union, as the kernel wrote them:
 * *nrec_out records of 1 + *words_out 64-bit words, the column index then the split's words; *records_out is released with pml_free */
int  pml_debug_column_splits(pml_ctx *ctx, const pml_alignment *gene, int nunion, const char *const *names_union, long long *nrec_out,
                             int *words_out, unsigned long long **records_out);
/* the kept splits that k_splitcost holds in LDS at a time (tests size a case beyond it) */
int  pml_congruence_ktile(void);

/* The reference's `-uniform_trim` (HandyConstants.java:26; PhylogenomicPipeline2.getAlignment :788-795 runs it on every gene before
 * filterForCongruence sees them) and MSATrimmer's two sibling filters, on the device (trim.hip).  Bytes are compared by identity
 * (no alphabet: 'a' and 'A' differ); n is the gene's OWN number of rows, nothing here involves a union of taxa, and n has no
 * bound.  For a column let seen1 = the set of bytes that occur, seen2 = the set of bytes that occur at least twice, shown = the
 * number of rows whose byte is neither '-' nor '?'.
 *   PML_TRIM_UNIFORM      trimUniformColumns (MSATrimmer.java:205-253): a column is kept iff getMinimumStepsPerSite
 *            (SequenceAlignment.java:673-682) is non-zero, i.e. iff it has more than one distinct Bipartition
 *            (getBipartitionsForAlignmentColumn :808-902).  With classes = |seen1 \ {'-','?'}|: kept iff classes >= 3, or classes == 2
 *            and shown < n.  Two classes that cover all n rows normalise to ONE bipartition (Bipartition.equals :292-303 compares the
 *            sides only), so the gap-free column AAAC or AACC is dropped while AAC- is kept: not what the name suggests, but
 *            the Java.  A column of nothing but '-' and '?' makes the Java dereference null; the library refuses it with PML_EPARSE
 *            and names gene and column (a deliberate difference).
 *   PML_TRIM_GAP_UNIFORM  trimUniformativeColumns (:141-203): only '-' is skipped, '?' is a character like any other; kept iff at
 *            least two distinct bytes other than '-' occur.  An all-'-' column is uniform and dropped.
 *   PML_TRIM_TOPOLOGICAL  trimTopologicallyUninformativeColumns (:264-351): only '-' is skipped; kept iff at least two distinct
 *            bytes other than '-' each occur at least twice, |seen2 \ {'-'}| >= 2.  All-'-' columns are dropped.  (Its
 *            uninformativeCount is a debug print and not part of the contract.)
 * In every mode the kept columns keep their order, rows and names are untouched, a gene may end with 0 columns, and gap_or_missing
 * is the numerator of getProportionGapOrMissing (SequenceAlignment.java:1074-1092): the '-' and '?' cells of the UNTRIMMED gene.
 * pml_trim_columns works through the genes in sub-batches that fit the HBM budget (0.85 of free HBM, or PML_HBM_BUDGET_MB): input,
 * output and flags of a sub-batch are resident together; a single gene that does not fit is PML_ENOMEM with the size. */
enum { PML_TRIM_UNIFORM = 0, PML_TRIM_GAP_UNIFORM = 1, PML_TRIM_TOPOLOGICAL = 2 };
typedef struct {
    int ngenes;
    int *ntax, *ncols, *nkept;        /* [G]: rows, columns before, columns kept */
    int **kept_cols;                  /* [G][nkept] ascending column indices */
    char ***rows;                     /* [G][ntax] the trimmed rows in input order, 0-terminated, owned by the result */
    long long *gap_or_missing;        /* [G] */
} pml_trim_result;
int  pml_trim_columns(pml_ctx *ctx, int ngenes, const pml_alignment *genes, int mode, pml_trim_result *result);
void pml_trim_result_free(pml_trim_result *result);
/* `-uniform_trim -congruence_filter` in one resident call: the genes are uploaded once, trimmed in HBM, and the congruence stage
 * runs on the trimmed device matrices.  Equals pml_trim_columns followed by pml_congruence_filter on the returned text, field for
 * field.  A gene trimmed to 0 columns is PML_EPARSE and names the gene (the Java divides by zero there).  The union of taxa is the
 * congruence filter's (at most 512); trim_result and congruence_result may each be NULL. */
int  pml_trim_congruence_filter(pml_ctx *ctx, int ngenes, const pml_alignment *genes, int mode, double trim_percent, int *keep_out,
                                pml_trim_result *trim_result, pml_congruence_result *congruence_result);
/* test door of k_colclass: one byte per column as the kernel wrote it: bit 0, bit 1, bit 2 = kept under PML_TRIM_UNIFORM,
 * PML_TRIM_GAP_UNIFORM, PML_TRIM_TOPOLOGICAL; bit 3 = only '-' / '?'.  flags_out: gene->nsites bytes */
int  pml_debug_column_flags(pml_ctx *ctx, const pml_alignment *gene, unsigned char *flags_out);
/* host-only, needs no context: the same bytes from the same decision function (csrc/trim.hpp) */
int  pml_trim_column_flags_host(const pml_alignment *gene, unsigned char *flags_out);
/* k_colclass and k_colgather launches on this context so far and, with cfg.profile = 1, summed HIP-event times in ms:
 * total_ms[0] = k_colclass, [1] = k_colgather, [2] = the host-to-device copies of the genes' bytes.  Never reset. */
int  pml_trim_stats(pml_ctx *ctx, long long *class_launches, long long *gather_launches, double *total_ms /* [3] */);

/* The reference's `-gblocks_trim` (PhyloPipeline.java:1121 sets it on the default track): MSATrimmer.trim (MSATrimmer.java:41-126) runs
 * `Gblocks <file> -o -b1=ceil(0.8 n) -b3=8 -b5=h` on every gene before -uniform_trim, the congruence filter and the trees.  Here the
 * block selection runs on the device (gblocks.hip).  PARITY WITH THE Gblocks BINARY IS UNPINNED: the reference holds no source of it
 * and the bundled 32-bit binary does not start, so the rule below is the published one (Castresana 2000 and the program's
 * documentation) and the tests pin the device against an independent restatement of this text.  Deliberate difference: residues are
 * counted by identity; the binary's similarity-matrix option, which its documentation describes as on by default for proteins, is
 * not applied (its matrix is not in the reference).
 *   A gene has n rows and L columns.  Bytes are compared by identity; '-' is the only gap byte, '?', 'X' and everything else are
 *   residues.  Parameters b1 <= b2 (conserved / flank thresholds), b3 (longest run of non-conserved columns tolerated), b4 (minimum
 *   block length), b0 (minimum length of an initial block), gaps.  A field that is 0 takes PEPR's value: b1 = (int)ceil(n * 0.8) in
 *   double (MSATrimmer.java:94-95), b2 = max(b1, 85 n / 100) in integer division (the program's documented default of 85 %; its
 *   rounding is unpinned), b3 = 8, b4 = b0 = 10, gaps = PML_GBLOCKS_GAPS_HALF.  Anything outside n / 2 < b1 <= b2 <= n, b3 >= 0,
 *   b4 >= 2, b0 >= 2 is PML_EINVAL.
 *   Per column, gaps(c) = its '-' bytes, top(c) = the largest count of one non-gap byte.  The column is a gap position under NONE iff
 *   gaps(c) > 0, under HALF iff 2 gaps(c) >= n, under ALL never.  Its class is 0 (non-conserved) if it is a gap position or
 *   top < b1, 2 (highly conserved) if top >= b2, else 1 (conserved).
 *   Every column starts selected; a block is a maximal run of selected columns.
 *   1. every maximal run of class-0 columns longer than b3 is deselected;
 *   2. in every block columns are deselected from each end until a class-2 column is reached (a block without one vanishes);
 *   3. every block shorter than b0 is deselected;
 *   4. inside the blocks every gap position is deselected, and every class-0 column joined to a gap position by an unbroken run of
 *      selected class-0 columns;
 *   5. every block shorter than b4 is deselected.
 * Kept columns keep their order, rows and names are untouched, a gene may end with 0 columns.  pml_gblocks_trim fills the
 * trim result of pml_trim_columns, gap_or_missing (the '-' and '?' cells of the untrimmed gene) included, and sub-batches under the HBM budget as
 * pml_trim_columns does (PML_HBM_BUDGET_MB; a single gene that does not fit is PML_ENOMEM with the size).  Selection, the kept
 * columns' prefix and the gather run on the device without a host step in between. */
enum { PML_GBLOCKS_GAPS_NONE = 1, PML_GBLOCKS_GAPS_HALF = 2, PML_GBLOCKS_GAPS_ALL = 3 };
typedef struct { int b1, b2, b3, b4, b0, gaps; } pml_gblocks_params;
/* host-only: PEPR's parameters for a gene of ntax rows */
int  pml_gblocks_defaults(int ntax, pml_gblocks_params *out);
int  pml_gblocks_trim(pml_ctx *ctx, int ngenes, const pml_alignment *genes, const pml_gblocks_params *params /* NULL = PEPR's */,
                      pml_trim_result *result);
/* test door: one byte per column as k_gbclass and k_gbselect wrote it: bits 0-1 = class, bit 2 = gap position, bit 4 = selected
 * after step 1, bit 5 = after steps 2 and 3, bit 6 = after step 4, bit 7 = kept.  flags_out: gene->nsites bytes */
int  pml_debug_gblocks_flags(pml_ctx *ctx, const pml_alignment *gene, const pml_gblocks_params *params, unsigned char *flags_out);
/* host-only, needs no context: the same bytes from the same functions (csrc/gblocks.hpp) with sequential scans */
int  pml_gblocks_flags_host(const pml_alignment *gene, const pml_gblocks_params *params, unsigned char *flags_out);
/* the columns k_gbselect scans at a time (tests place their cases across this boundary) */
int  pml_gblocks_chunk(void);
/* k_gbclass and k_gbselect launches on this context so far and, with cfg.profile = 1, summed HIP-event times in ms:
 * total_ms[0] = k_gbclass, [1] = k_gbselect, [2] = the host-to-device copies.  The gather counts in pml_trim_stats.  Never reset. */
int  pml_gblocks_stats(pml_ctx *ctx, long long *class_launches, long long *select_launches, double *total_ms /* [3] */);
/* The trimming stages in the reference's order (PhylogenomicPipeline2.getAlignment :737-806) in one resident call with one upload:
 * Gblocks (use_gblocks != 0; gb as for pml_gblocks_trim), then the column filter (mode, -1 = none), then the congruence filter
 * (trim_percent, 0 = none; keep_out is needed then).  Each stage reads the matrices the stage before left in HBM.  Equals
 * pml_gblocks_trim, pml_trim_columns and pml_congruence_filter run one after the other on the returned text, field for field.  A
 * gene that a stage empties while another stage follows is PML_EPARSE and names gene and stage.  All genes are resident together
 * (PML_ENOMEM otherwise); no stage at all is PML_EINVAL; each result pointer may be NULL. */
int  pml_trim_pipeline(pml_ctx *ctx, int ngenes, const pml_alignment *genes, const pml_gblocks_params *gb, int use_gblocks, int mode,
                       double trim_percent, int *keep_out, pml_trim_result *gb_result, pml_trim_result *trim_result,
                       pml_congruence_result *congruence_result);

/* The gene homoplasy test of ConcatenatedSequenceAlignment.java:65-425: per-column parsimony steps of the concatenation on a tree,
 * the least steps a column can take, per-gene totals, and for every gene a randomisation threshold (genesteps.hip).  In the
 * reference this is dead code: its one input, setStepsPerSite (SequenceAlignment.java:1033), has no caller, because neither RAxML
 * nor FastTree reports per-site steps.  Here the engine's own Fitch pass supplies them.
 *   genes     as for pml_jackknife.  The concatenation is MSAConcatenator's: the sorted union of the genes' taxa, the genes in the
 *             given order, a taxon a gene lacks is a row of '?'.  Nothing is concatenated as text.
 *   newick    exactly the union's taxa; a rooted binary tree is unrooted first.  A polytomy other than a trifurcation at the top, a
 *             missing or an extra taxon: PML_EPARSE.
 *   steps[c]  the Fitch length of column c: tip sets are the state sets of the alignment codes, so '?', '-' and X are all 20
 *             states, B = N|D, Z = Q|E, and an absent taxon is all states.
 *   min_steps[c]  getMinimumStepsPerSite (SequenceAlignment.java:673-682 with getBipartitionsForAlignmentColumn :808-902): the
 *             column's distinct Bipartitions less one.  Bytes are compared by identity over the n rows of the union.  With classes =
 *             the distinct bytes other than '-' and '?' and shown = the rows showing neither: classes - 1 - [classes == 2 and
 *             shown == n], the quirk PML_TRIM_UNIFORM documents (two classes that cover all rows are ONE bipartition); shown == n
 *             needs the gene to hold every taxon of the union.  A column of nothing but '-' and '?' makes the Java dereference
 *             null: PML_EPARSE naming gene and column.
 *   totals    (:65-103) gene_steps and gene_beyond are the Java's int sums kept in 64 bits; gene_ratio is the Java's sequential
 *             float sum of (float)steps / (float)(min_steps + 1) in column order.
 * The genes are worked through in sub-batches that fit the HBM budget (0.85 of free HBM, or PML_HBM_BUDGET_MB); a single gene that
 * does not fit is PML_ENOMEM with the size. */
typedef struct {
    int ngenes, ntax;
    char **names;                     /* [ntax] the sorted union */
    long long ncols;                  /* sum of the genes' columns */
    long long *col_start;             /* [ngenes + 1] the Java's startStops */
    int *steps, *min_steps;           /* [ncols] */
    long long *gene_steps, *gene_beyond;   /* [ngenes] */
    float *gene_ratio;                /* [ngenes] */
} pml_gene_steps_result;
int  pml_gene_steps(pml_ctx *ctx, int ngenes, const pml_alignment *genes, const char *newick, pml_gene_steps_result *out);
void pml_gene_steps_result_free(pml_gene_steps_result *result);
/* The randomisation thresholds (:141-425).  Gene g's replicate is a sample of as many columns as g has, drawn from its domain: the
 * columns of every gene h != g with !mask[h], in column order, U of them.  threshold[g] = the ascending-sorted replicate sums at
 * index reps - k, k = (int)ceil(reps * alpha); n_ge[g] = the replicates whose sum is >= the gene's observed total.
 *   statistic  the per-column table: steps, steps - min_steps, or the float ratio above
 *   replace    1 = with replacement, 0 = without
 *   multiple   > 0 and U < len_g * multiple: threshold[g] = -1 and n_ge[g] = -1, no error (the Java's "enough columns" rule)
 * The Java's five methods: :141-176 = {RAW, 0, 0, no mask}; :178-213 = {BEYOND_MIN, 0, 0, no mask}; :240-307 (the current one) =
 * {BEYOND_MIN, 1, 3, mask}; :309-365 (...OLD) = {BEYOND_MIN, 0, 2, mask}; :367-425 = {MIN_RATIO, 0, 2, mask}.
 * PML_EINVAL: k outside [1, reps] (the Java indexes out of bounds); replace == 0, multiple == 0 and U < len_g (the Java loops for
 * ever), naming the gene; ncols >= 2^31 or ngenes * reps >= 2^31.
 * The draws are the library's own: the Java's generator is an unseeded java.util.Random, so its definitions are matched, not its
 * stream.  base = (seed + 1) * 0x9E3779B97F4A7C15, key = base + ((g * reps + b) << 32) for replicate b.  With replacement draw j is
 * the domain index ((mix64(key + j) >> 32) * U) >> 32.  Without replacement draw j is perm(mix64(key), U, j), a keyed bijection of
 * [0, U): h = max(1, (bitlength(U - 1) + 1) / 2), x = L << h | R, four rounds (L, R) = (R, L ^ (mix64(K + (r << 40) + R) & (2^h - 1))),
 * repeated while x >= U.  It yields a uniformly random len_g-subset of the domain, as the Java's rejection loop does; only the
 * subset enters the sum.  int sums are exact, float sums are the Java's sequential chain in draw order. */
enum { PML_STEPS_RAW = 0, PML_STEPS_BEYOND_MIN = 1, PML_STEPS_MIN_RATIO = 2 };
typedef struct {
    int statistic, replace, multiple, reps;
    double alpha;
    unsigned long long seed;
    const unsigned char *mask;        /* [ngenes] or NULL */
} pml_step_threshold_opts;
int  pml_step_thresholds(pml_ctx *ctx, const pml_gene_steps_result *result, const pml_step_threshold_opts *opts, double *threshold /* [ngenes] */,
                         long long *n_ge /* [ngenes], may be NULL */);
/* host-only, needs no context: the concatenation columns that replicate `rep` of `gene` draws, in draw order, from the same draw
 * functions (csrc/genesteps.hpp).  cols_out: the gene's number of columns.  A gene under the -1 rule: PML_EINVAL */
int  pml_step_draws_host(const pml_step_threshold_opts *opts, int ngenes, const long long *col_start, int gene, int rep, long long *cols_out);
/* test door of k_steps_resample: the kernel's sums of one gene, alone in its launch, unsorted.  sums: opts->reps values */
int  pml_debug_step_replicates(pml_ctx *ctx, const pml_gene_steps_result *result, const pml_step_threshold_opts *opts, int gene, double *sums);
/* launches on this context so far and, with cfg.profile = 1, summed HIP-event times in ms: [0] = k_fitch_sitesteps, [1] =
 * k_steps_expand, [2] = k_colminsteps (each one per sub-batch of pml_gene_steps), [3] = k_steps_resample, [4] = k_steps_table (each
 * one per pml_step_thresholds / pml_debug_step_replicates).  Never reset. */
int  pml_gene_steps_stats(pml_ctx *ctx, long long *launches /* [5] */, double *total_ms /* [5] */);

/* TreeComparison's `-rf` and `-tree_dist` legs (TreeComparison.java:48-50, compareAllvsAll :267-288) for a whole set of trees:
 * every pair (i, j), i < j, tree 1 = i, on the device (treecmp.hip).  The trees are given as Newick text and must all have the
 * same leaf labels (PML_EINVAL otherwise; at most 512 leaves, at least 3).
 *   model    what the Java compares is TreeParser.parseTreeString(BasicTree.getTreeString(useLengths, true)): one branch per node
 *            below the top level, pendant branches included; a top level of two becomes ONE branch with the sum of the two
 *            lengths, a top level of three becomes three branches; any other top level leaves the Java without a tree and is
 *            PML_EINVAL here, as is a node with a single child (the Java's round trip corrupts its leaf's name).  A branch without
 *            a length has length 0; use_lengths = 0 reads every length as 0; an inner node's label is its support and enters no
 *            value.  Tree.getBranches() has no defined order in the Java (a HashSet of objects without hashCode); this library
 *            uses the order in which TreeParser creates the branches: nodes in ascending index of the round-tripped text
 *            (a node's leaves before its inner children; leaves in text order, inner nodes in the order of their ')'), then the
 *            top-level branch or branches.  Only the rounding of the sums and, for a repeated split, the choice of the counterpart
 *            depend on it.
 *   rf_legacy       Tree.getRobinsonFouldsDistance (Tree.java:589-603): (|union| - |intersection|) / 4 over the sets that hold
 *                   BOTH leaf sets of every branch = (dA + dB - 2 shared) / 2 over distinct splits, pendant ones included.
 *   rf_bipartition  AdvancedTree.getRobinsonFouldsDistance (AdvancedTree.java:1460-1483): the same over non-trivial splits.
 *   rf_splits       pml_rf_distance of the two texts: multifurcations resolved as Tree::parse resolves them.
 *   branch_dist     getBranchDistance (TreeComparison.java:607-747): lengths over the tree's maximum; a branch's counterpart is
 *                   the LAST branch of tree 2 with its split; sqrt(r) / sqrt(ss1 + ss2).  NaN when every length is 0.
 *   discrepant_dist getDiscrepantBranchDistance (:756-810): raw lengths, unmatched branches only.
 * The sums are accumulated on the device in the Java's order without fused multiply-adds; sqrt and the division are the host's.
 * The diagonal holds 0 in the RF arrays and the formula's value of a tree against itself in the distances.  window = w > 0
 * computes only |i - j| <= w (compareSlidingWindow :241-265, rollingComparison :457-466 are bands of the matrix); other entries
 * hold -1 / NaN.  The trees' records stay in HBM for the call and the pair outputs are produced in blocks of rows that fit the
 * budget (0.85 of free HBM, or PML_HBM_BUDGET_MB, which may be fractional here); a set whose records plus one row do not fit
 * is PML_ENOMEM with the sizes.  compareBranchSupports (:374-454) is not part of this. */
enum { PML_TC_RF_LEGACY = 1, PML_TC_RF_BIPARTITION = 2, PML_TC_RF_SPLITS = 4, PML_TC_BRANCH_DIST = 8, PML_TC_DISCREPANT_DIST = 16 };
typedef struct {
    int window;                       /* 0 = all pairs */
    int use_lengths;                  /* TreeComparison's -use_lengths (the Java's default is true) */
    int want;                         /* PML_TC_* bits of the arrays to produce; 0 = all */
} pml_tree_compare_opts;
typedef struct {
    int nrows, ncols, ntax;           /* T x T (pml_tree_compare) or 1 x T (pml_tree_compare_one); row-major */
    int *rf_legacy, *rf_bipartition, *rf_splits;      /* NULL when not wanted */
    double *branch_dist, *discrepant_dist;
    long long row_blocks;             /* k_tree_pairs launches of the call */
    long long resident_bytes, row_bytes;              /* HBM held by the records; HBM per row of pair outputs */
} pml_tree_compare_result;
int  pml_tree_compare(pml_ctx *ctx, int ntrees, const char *const *newicks, const pml_tree_compare_opts *opts /* NULL: all pairs, lengths, all arrays */,
                      pml_tree_compare_result *out);
/* calculateTreeDistances (:557-565): the standard tree (tree 1) against each of the ntrees comparison trees; window is ignored */
int  pml_tree_compare_one(pml_ctx *ctx, const char *standard_newick, int ntrees, const char *const *newicks, const pml_tree_compare_opts *opts,
                          pml_tree_compare_result *out);
void pml_tree_compare_result_free(pml_tree_compare_result *result);
/* test door: the split records of a tree set as the kernels see them.  Tree t owns records first[t] .. first[t + 1] - 1; its
 * first nreal[t] are its branches in branch order, the rest are the splits that resolving its multifurcations adds (rf_splits).
 * split_words: W words per record over the sorted names, normalised (the side with fewer leaves, on a tie the side holding
 * taxon 0); flags: 1 = a branch, 2 = trivial, 4 = the last record of its tree with its split; split_id: the index of the first
 * record of the call with the same split. */
typedef struct {
    int ntrees, ntax, words;
    char **names;
    long long nrecords, *first;       /* [T + 1] */
    int *nreal;                       /* [T] */
    unsigned long long *split_words;  /* [nrecords][W] */
    double *length, *length_norm;     /* [nrecords] */
    int *flags, *split_id;            /* [nrecords] */
} pml_tree_splits;
int  pml_debug_tree_splits(pml_ctx *ctx, int ntrees, const char *const *newicks, int use_lengths, pml_tree_splits *out);
void pml_tree_splits_free(pml_tree_splits *out);
/* test door: what k_tree_pairs and k_tree_sums give for chosen pairs (i <= j): counts_out[p][7] = shared splits, shared
 * non-trivial splits, shared splits of the resolved trees, distinct and distinct non-trivial splits of i, the same of j;
 * sums_out[p][6] = r, sumOfSquaresTree1, sumOfSquaresTree2 of getBranchDistance, then of getDiscrepantBranchDistance */
int  pml_debug_tree_pair_sums(pml_ctx *ctx, int ntrees, const char *const *newicks, int use_lengths, int npairs, const int *pairs /* [npairs][2] */,
                              long long *counts_out, double *sums_out);

/* The reference's NeighborMasher (util/NeighborMasher.java): from a few ingroup genomes and a pool of candidate genomes it picks the
 * ingroup's expansion and the outgroups and builds NJ trees of both from `mash sketch` / `mash dist` genome distances
 * (TreeBuilder.getNJTreeString with TreeBuilder.DISTANCE = pml_nj_from_matrix, PML_NJ_DISTANCE, PML_NJ_TREE).  Here the sketches and
 * the pair counts are computed on the device (mash.hip).  PARITY WITH THE mash BINARY IS UNPINNED: the reference holds neither a mash
 * binary nor its source, so the rule below is the published one (Ondov et al. 2016 and the program's documentation) and the tests pin
 * the device against an independent restatement of this text (tests/mash_ref.py).  Part of what is unpinned: NeighborMasher reads the
 * distance from mash's text, which is taken to carry six significant digits; `digits` = 6 feeds strtod("%.6g") of the distance to
 * the selection and to NJ, `digits` = 0 the double itself.  mash's p-value, -i, amino-acid alphabets and .msh files are not built.
 *   windows    A genome is a list of records, each a byte string; 'a'..'z' read as upper case.  A window is k consecutive bytes of ONE
 *              record, 1 <= k <= 32, valid iff all of them are in ACGT.  A record shorter than k gives none; an empty record is legal.
 *   canonical  the smaller, as byte strings, of the window and its reverse complement; the window itself when they are equal (even
 *              k, e.g. ACGT).
 *   hash       h1 of MurmurHash3_x64_128 over the k canonical bytes with seed 42: c1 = 0x87c37b91114253d5, c2 = 0x4cf5ad432745937f,
 *              h1 = h2 = seed; per 16-byte block, k1 and k2 read little-endian: k1 *= c1, k1 = rotl(k1, 31), k1 *= c2, h1 ^= k1,
 *              h1 = rotl(h1, 27), h1 += h2, h1 = h1 * 5 + 0x52dce729; k2 *= c2, k2 = rotl(k2, 33), k2 *= c1, h2 ^= k2, h2 = rotl(h2, 31),
 *              h2 += h1, h2 = h2 * 5 + 0x38495ab5.  Tail: bytes 8..14 little-endian into k2, mixed as above without the h2 rotation,
 *              add and multiply; bytes 0..7 into k1 likewise.  Finish: h1 ^= len, h2 ^= len, h1 += h2, h2 += h1, h1 = fmix(h1),
 *              h2 = fmix(h2), h1 += h2, h2 += h1; fmix(x): x ^= x >> 33, x *= 0xff51afd7ed558ccd, x ^= x >> 33,
 *              x *= 0xc4ceb9fe1a85ec53, x ^= x >> 33.  For k <= 16 (4^k <= 2^32) only the low 32 bits of h1 are kept.
 *              Check vectors: "The quick brown fox jumps over the lazy dog", seed 0: h1 = e34bbc7bbc071b6c, h2 = 7a433ca9c49a9347;
 *              the empty string, seed 0: 0, 0; "ACGTACGTACGTACGTACGTA", seed 42: h1 = b4e9c495b633d387.
 *   sketch     the ascending list of the min(s, D) smallest distinct values of a genome, D = its distinct values, s >= 1.  A genome
 *              without a valid window has an empty sketch.
 *   pair       for sketches a, b and size s:  i = j = common = denom = 0;  while denom < s and i < |a| and j < |b|:  a[i] < b[j]: i++;
 *              b[j] < a[i]: j++;  else i++, j++, common++;  denom++.  Then, if denom < s: denom = min(s, denom + |a| - i + |b| - j).
 *              common = the shared values among the s smallest of the union, denom = min(s, |union|): the device's two integers.
 *   distance   on the host, in double: 0 if common == denom (two empty sketches included), else 1 if common == 0, else
 *              min(1, -log(2 j / (1 + j)) / k) with j = common / denom.
 * On the device a window that is not valid is marked with 2^64 - 1, so for k > 16 a valid window whose h1 IS 2^64 - 1 (one in 2^64)
 * is dropped there and kept by the host doors: the one place where the two can differ.
 * The Java half is source and pinned by reading, ties between equal distances excepted: the Java's HashSet / HashMap iteration
 * leaves their order to the JVM, here they follow input order (after the stable sorts).
 *   expandIngroup :281-324   a candidate's distance is the maximum of its distances to the ingroup taxa; a stable ascending sort;
 *              candidates below 1.0 whose name is not an original ingroup taxon's are added until the target size is reached.
 *   getMaxDistanceForEachOutgroupToIngroupSketch :738-783   every pool genome, with its maximum distance to the (final) ingroup.
 *   getIngroupPairDistances :855-867 with StatisticsUtilities :158-173, :831-840, :938-949   mean (NaN entries skipped), standard
 *              deviation with n - 1 (NaN for a single pair, -0.0 for none), maximum (NaN for none).
 *   selectOutgroupCandidates :483-568   the threshold is max ingroup distance + sd * 0 (NaN when sd is NaN: then nothing is
 *              acceptable); candidates in stable ascending order; one below 1.0 and above the threshold is acceptable, one below 1.0
 *              and not above it is too near; the loop ends when `count` DISTINCT acceptable distances are met (so the last distance
 *              contributes its first candidate only); up to `count` candidates by ascending distance are selected; when none is
 *              acceptable, the first candidate of the largest too-near distance, one only.
 *   run :112-195   the ingroup tree is built when !outgroup_only and expand_ingroup > 3, the second tree when neither flag is set
 *              and expand_ingroup + the selected outgroups > 3: both conditions read the OPTION, not the ingroup's size, as the Java
 *              does (with the default 0 no ingroup tree is written).  Where the Java would then hand NJ fewer than 4 taxa (it writes
 *              "null") the tree is left out.  buildNJTreeOfTaxa :623-635 orders the taxa outgroups first.
 * Not built: rooting (AdvancedTree.setOutGroup + getTreeString :637-640): the second tree is the UNROOTED NJ tree with the outgroup
 * taxa first.  A genome is given with explicit lengths; its bytes may be anything. */
typedef struct {
    int nrecords;
    const char *const *records;       /* [nrecords] bytes, not terminated */
    const long long *lengths;         /* [nrecords] */
} pml_genome;
/* the window starts k_mash_hash stages at a time, and the sketch values k_mash_pairs takes at a time (tests aim at these boundaries) */
int  pml_mash_tile(void);
int  pml_mash_chunk(void);
/* Genomes to sketches: values_out [ngenomes][s] (row g: len_out[g] ascending values, then zeros).  The caller may keep them between
 * runs, the role of the reference's -outgroup_sketch file.  Genomes are hashed in sub-batches that fit the HBM budget (0.85 of free
 * HBM, or PML_HBM_BUDGET_MB); a single genome that does not fit, or one of 2^31 bytes or more, is PML_ENOMEM.  k outside 1..32 and
 * s < 1 are PML_EINVAL.  Selection: a histogram of the values' leading 12 bits gives every genome a cut, the values under it are
 * compacted, sorted (rocPRIM's segmented radix sort) and deduplicated; a genome with fewer than s distinct values under a cut that
 * is not yet everything gets a cut at least twice as wide and its sub-batch is repeated (pml_mash_stats counts these). */
int  pml_mash_sketch(pml_ctx *ctx, int ngenomes, const pml_genome *genomes, int k, int s, unsigned long long *values_out, int *len_out);
/* every pair of two sets of host sketches ([n][s] rows as pml_mash_sketch leaves them; each ascending and distinct, else PML_EINVAL):
 * common_out, denom_out, distance_out are na x nb, row major; each may be NULL.  digits as above (0 = the double) */
int  pml_mash_dist(pml_ctx *ctx, int na, const unsigned long long *a_values, const int *a_len, int nb, const unsigned long long *b_values, const int *b_len,
                   int k, int s, int digits, int *common_out, int *denom_out, double *distance_out);
/* the same from genomes: the sketches never leave HBM */
int  pml_mash_distances(pml_ctx *ctx, int na, const pml_genome *a, int nb, const pml_genome *b, int k, int s, int digits, int *common_out, int *denom_out,
                        double *distance_out);
/* test door: what k_mash_hash wrote for one genome: one value per byte of every record in order (sum of lengths values), 2^64 - 1
 * where no valid window starts */
int  pml_debug_mash_hashes(pml_ctx *ctx, const pml_genome *genome, int k, unsigned long long *values_out);
/* test door: on != 0 makes every cut take everything (the full-sort baseline of tools/measure_mash.py) */
int  pml_debug_mash_full_sort(pml_ctx *ctx, int on);
/* launches[5] = k_mash_hash, k_mash_cut, k_mash_compact, k_mash_unique, k_mash_pairs on this context so far; with cfg.profile = 1
 * total_ms[4] = the uploads, k_mash_hash, the selection (cut, compaction, sort, deduplication), k_mash_pairs; *repeats = sub-batches
 * repeated with a raised cut.  Never reset. */
int  pml_mash_stats(pml_ctx *ctx, long long *launches, double *total_ms, long long *repeats);
/* host-only, no context: the rule above over bytes (csrc/mash_host.cpp).  pml_mash_hashes_host = pml_debug_mash_hashes' values */
int  pml_mash_murmur3(const void *key, long long len, unsigned seed, unsigned long long out[2]);
int  pml_mash_hashes_host(const pml_genome *genome, int k, unsigned long long *values_out);
int  pml_mash_sketch_host(const pml_genome *genome, int k, int s, unsigned long long *values_out /* [s] */, int *len_out);
int  pml_mash_pair_host(const unsigned long long *a, int na, const unsigned long long *b, int nb, int s, int *common_out, int *denom_out);
double pml_mash_distance_of(int common, int denom, int k, int digits);
/* host-only: the Java's routines on indices.  d is [n_pool][n_in], the pool genomes' distances to the ingroup taxa */
int  pml_mash_candidate_distances(int n_in, int n_pool, const double *d, double *cand_out /* [n_pool] */);
int  pml_mash_expand_ingroup(int n_in, int n_pool, const double *d, const unsigned char *pool_is_ingroup /* [n_pool] or NULL */, int target,
                             int *added_out /* [n_pool] pool indices in the order added */, int *nadded_out);
int  pml_mash_pair_stats(int n, const double *d, double out3[3] /* mean, sd, max */);
int  pml_mash_select_outgroup(int n, const double *cand, double max_ingroup, double sd, int count, int *selected_out /* [n] */, int *nselected_out);
/* NeighborMasher.run() as one call.  PML_EINVAL with a message: k, s as above, an empty name list (the pool may be empty only with
 * ingroup_only and no expansion), a taxon name twice in one list, and -- here only -- a genome whose sketch is empty.  A pool genome
 * that carries an ingroup taxon's name is never added by the expansion. */
typedef struct {
    int n_ingroup, n_pool;
    const pml_genome *ingroup, *pool;
    const char *const *ingroup_names, *const *pool_names;
    int k, s;                         /* the Java's defaults: 21, 100000 */
    int outgroup_count;               /* 3 */
    int expand_ingroup;               /* 0 */
    int ingroup_only, outgroup_only;
    int digits;                       /* 6 = as read from mash's text, 0 = the double */
} pml_neighbor_masher_opts;
typedef struct {
    int n_ingroup; int *ingroup;      /* the final ingroup: i < opts->n_ingroup = ingroup genome i, else pool genome i - opts->n_ingroup */
    int n_outgroup; int *outgroup;    /* pool indices, in the order selected */
    int n_pool; double *candidate_distance;            /* [n_pool] maximum distance to the final ingroup; NULL with ingroup_only */
    double mean, sd, max;             /* of the final ingroup's pair distances (NaN with ingroup_only) */
    int n_taxa; int *taxa;            /* the outgroups, then the ingroup, indexed as `ingroup` is */
    double *distance; int *common, *denom;             /* [n_taxa][n_taxa] as fed to NJ: symmetric from the upper triangle, 0 diagonal */
    int *sketch_len;                  /* [opts->n_ingroup + opts->n_pool] */
    char *ingroup_tree, *rooted_tree; /* NULL where run() builds none; the ingroup tree is NJ of the trailing block of `distance` */
} pml_neighbor_masher_result;
int  pml_neighbor_masher(pml_ctx *ctx, const pml_neighbor_masher_opts *opts, pml_neighbor_masher_result *result);
void pml_neighbor_masher_result_free(pml_neighbor_masher_result *result);

/* ---- Homolog groups: Markov clustering of the hit graph (PhyloPipeline.java:357-406) ----
 * What the reference does between its all-vs-all search and its trees: filterHitPairFile :989-1024 or filterForBidirectional
 * :911-987, `mcl <hits> --abc -I 1.5` (runMCL :882-909), one set_<k>.faa per line of mcl's output (SequenceSetExtractor) and
 * the choice of the sets that become genes (SequenceSetProviderImpl, PhylogenomicPipeline2.createInputSequenceSetProvider
 * :564-605).  PINNED: clusters, their order and their members' order equal mcl 09-308's on the committed cases
 * (tests/golden/mcl_cases.json, written by tests/golden/make_mcl_cases.py beside the binary); the filters and the selection are
 * restated from the Java source.  The rule:
 *   nodes      the labels of the table in order of first appearance, id1 before id2 on a line
 *   arcs       `a b w`, a != b, sets G[a][b] and G[b][a] to the larger of their present value and w (a mirror with a max
 *              combine).  A self hit only makes its label a node.  A weight that is not finite or is <= 0 is PML_EINVAL
 *   loops      G[j][j] = the largest entry of column j, 1 where the column is otherwise empty; M = G, every column over its sum
 *   iteration  at most max_iter (10000) times: M <- M M; entries below 1 / prune_inverse (10000) become 0 and the columns are
 *              renormalised; chaos = max_j (max_i M_ij - sum_i M_ij^2); M_ij <- M_ij^inflation and the columns are renormalised;
 *              stop when chaos < chaos_eps (1e-3)
 *   reading    attractors are the i with M_ii > 0; attractors a, b with M_ab > 0 are one system; node j joins the system of the
 *              attractor row with the largest M_aj, the lowest index of equals (a node of a matrix without attractors stays alone)
 *   order      clusters by size, largest first, ties to the lower smallest member; members ascending by index.  mcl's text is
 *              one cluster per line, labels joined by tabs; set_<k>.faa is line k (from 0), so the order is part of the contract
 *   components connected components of G are clustered independently (the matrix is block diagonal); the iteration count
 *              reported is the slowest component's
 * NOT BUILT: mcl's selection and recovery pruning (-S 1100 -R 1400 -pct 90), which act only on columns of more than 1100 entries
 * -- parity is claimed for components up to that size only; mcl's other input modes; sparse expansion (every component is a dense
 * f64 matrix: one of n nodes takes 16 n^2 bytes rounded up to tiles, and one that does not fit the HBM budget -- 0.85 of free HBM,
 * or PML_HBM_BUDGET_MB -- is PML_ENOMEM with its size in the message).
 * Device classes (pml_mcl_class_limits): components of up to limits[0] nodes run packed, four to a workgroup, one wavefront each;
 * up to limits[1] one workgroup each, both with the matrix in LDS and the whole iteration inside ONE launch; larger ones in HBM,
 * a tiled expansion (tile limits[2]) and a column kernel per iteration, the host reading one flag per component between them.
 * All arithmetic is f64, the expansion on v_mfma_f64_16x16x4_f64. */
typedef struct pml_mcl_opts {
    double inflation, prune_inverse, chaos_eps;       /* 0 = 1.5, 10000, 1e-3 */
    int max_iter, pad;                                /* 0 = 10000 */
} pml_mcl_opts;
/* the integer-level call: nodes 0 .. n-1, arcs (a[i], b[i], w[i]).  cluster_of_out[n] numbers the clusters in output order */
int  pml_mcl_cluster(pml_ctx *ctx, int n, long long narcs, const int *a, const int *b, const double *w, const pml_mcl_opts *opts,
                     int *cluster_of_out, int *nclusters_out, int *iters_out);
/* the same rule in plain C++ loops, no context (csrc/mcl_host.cpp): the CPU tests' subject and the timing baseline */
int  pml_mcl_cluster_host(int n, long long narcs, const int *a, const int *b, const double *w, const pml_mcl_opts *opts,
                          int *cluster_of_out, int *nclusters_out, int *iters_out);
/* The hit table to gene sets.  score_field 11: the table is BLAST's tabular output and goes through filterHitPairFile, or with
 * `bidirectional` through filterForBidirectional(file, 11); score_field 2: it already is `id1 id2 score` and is clustered as
 * it stands (bidirectional must be 0).  Selection runs when taxon_labels is given: label taxon_labels[i] belongs to taxon
 * taxon_of[i] (a clustered label without an entry is PML_EINVAL): clusters with min_taxa <= members <= max_taxa (a sequence
 * count); with rep_only those in which no taxon occurs twice; then, if more than target_min_gene remain, for t = min_taxa + 1 ..
 * target_ntax: when at least target_min_gene clusters have >= t distinct taxa, those with fewer are dropped. */
typedef struct {
    const char *table; long long table_bytes;
    int score_field, bidirectional;
    pml_mcl_opts mcl;
    int ntaxon_labels; const char *const *taxon_labels; const int *taxon_of;
    int min_taxa, max_taxa, rep_only, target_ntax, target_min_gene;
} pml_homolog_groups_opts;
typedef struct {
    int nlabels; char **labels;                       /* the nodes */
    int nclusters; long long *cluster_off;            /* [nclusters + 1] into members */
    int *members;                                     /* [nlabels] node indices, cluster by cluster in output order */
    char *mcl_text;                                   /* mcl's output file */
    int nkept; int *kept;                             /* cluster indices the selection keeps, ascending (all without taxon_labels) */
    int ncomponents, iterations;
    char *filtered_text;                              /* the <hits>_filtered or <hits>_bidir file; NULL with score_field 2 */
} pml_homolog_groups_result;
int  pml_homolog_groups(pml_ctx *ctx, const pml_homolog_groups_opts *opts, pml_homolog_groups_result *result);
void pml_homolog_groups_result_free(pml_homolog_groups_result *result);
/* host-only, no context.  The filters return malloc'ed text (pml_free).  filterHitPairFile: fields 0, 1 and 11 of the lines
 * with more than one field (a line with 2 .. 11 fields, the Java's exception, is PML_EINVAL).  filterForBidirectional: only
 * lines with more than score_field fields count; pairs are unordered, self pairs included; the first sighting of a pair stores
 * new Float(field), the next writes `id1 id2 <field text>` and `id2 id1 <Float.toString(stored)>` and forgets the pair, so a
 * third sighting stores again.  Float.toString is restated for finite values: the shortest decimal that round-trips the f32,
 * at least one digit behind the point, the E form outside [1e-3, 1e7); the known JDK cases that are not shortest are NOT
 * reproduced. */
int  pml_hits_filter_host(const char *table, long long table_bytes, char **text_out);
int  pml_hits_bidirectional_host(const char *table, long long table_bytes, int score_field, char **text_out);
int  pml_homolog_select_host(int nclusters, const long long *cluster_off, const int *members, const int *taxon_of_node, int min_taxa, int max_taxa,
                             int rep_only, int target_ntax, int target_min_gene, int *kept_out /* [nclusters] */, int *nkept_out);
/* test doors.  limits_out[4] = the packed class's and the LDS class's largest component, the expansion tile, 0 */
int  pml_mcl_class_limits(int *limits_out);
/* nsteps iterations (no convergence test) of ONE dense component in class force_class (0 packed, 1 LDS, 2 HBM; PML_EINVAL when n
 * exceeds the class): matrix_in / matrix_out are n x n, row major ([i * n + j] = M_ij), matrix_in column stochastic;
 * *chaos_out = the last iteration's chaos */
int  pml_debug_mcl_steps(pml_ctx *ctx, int n, const double *matrix_in, const pml_mcl_opts *opts, int nsteps, int force_class, double *matrix_out,
                         double *chaos_out);
/* launches[8] = k_mcl_fill, k_mcl_packed, k_mcl_lds, k_mcl_expand, k_mcl_inflate, k_mcl_flag, k_mcl_read, sub-batches on this
 * context so far; with cfg.profile = 1 total_ms[4] = uploads and fill, the packed class, the LDS class, the HBM class (its host
 * loop included, by HIP events).  Never reset. */
int  pml_mcl_stats(pml_ctx *ctx, long long *launches, double *total_ms);

/* ---- Homology search: the all-vs-each Smith-Waterman hit table ----
 * The table pml_homolog_groups starts from.  The reference makes it in PhyloPipeline.runBlast (:1061-1077) through BlastRunner
 * (alignment/BlastRunner.java:539-599): `blastall -p blastp -d <genome g> -i <all proteins> -e 0.1 -v 1 -b 1 -m 8`, once per target
 * genome.  Neither a BLAST binary nor its source is in the reference, so PARITY WITH blastall IS UNPINNED: this is the exact
 * search BLAST approximates, every protein against every protein of every genome, and only the fields everything downstream
 * reads (query id, subject id, bit score: filterHitPairFile :989-1024, filterForBidirectional :911-987) are claimed.
 * Input: G genomes in the caller's order, each an ordered list of proteins.  A label is the first whitespace-delimited token of
 * labels[i].  Residues are upper-cased; the codes of the BLOSUM62 table as loaded (pml_pairwise_scores' table576, same order:
 * ARNDCQEGHILKMFPSTWYV B Z X) map to themselves, J O U map to X; `-` or any other byte is PML_EINVAL naming protein and position.
 * A protein of length 0 is neither query nor subject; a length above 65 535 is PML_EINVAL.
 * Score: Smith-Waterman with affine gaps, a gap of length k costs open + k * extend (defaults 11 and 1, blastp's "existence
 * 11, extension 1"):  E[i][j] = max(E[i][j-1] - ext, H[i][j-1] - open - ext), F[i][j] the same along i,
 * H[i][j] = max(0, H[i-1][j-1] + s(q_i, t_j), E[i][j], F[i][j]), S = max H.  Exact integers (int32) on the device, in the host
 * twin and in tests/sw_ref.py.  Table entries must fit int8.
 * Selection (-v 1 -b 1 per blastall run): for every query q (every protein of every genome) and every target genome g (its own
 * included) the winner is the subject of g with the largest S, ties to the lowest position in g's order.  hits_per_query other
 * than 0 / 1 is PML_EINVAL.
 * Statistics, on the host in f64 from the integer S: bits = (lambda S - ln K) / ln 2, E = K m N exp(-lambda S), m the query
 * length, N the total residues of genome g; defaults lambda 0.267, K 0.041 (BLOSUM62, 11/1, gapped).  A winner is a hit when
 * E <= evalue (default 0.1, the Java's evalueCutoff) and S > 0.
 * NOT BUILT: SEG masking, composition-based statistics, effective-length correction (no length adjustment is made), more than
 * one HSP per pair, hits_per_query > 1, a k-mer prefilter or any non-exhaustive mode.
 * Table: one line per hit, in the order of BlastRunner.getResults with one query set: target genome by target genome, within a
 * target the queries in genome order, then file order.  Twelve tab-separated fields `qlabel slabel pident length mismatch
 * gapopen qstart qend sstart send evalue bits`, evalue as %.2e, bits as %.1f.  With traceback = 0 fields 2..9 are `0`.  With
 * traceback = 1 the host fills them from one optimal alignment of each hit (a host loop over the hits only): the end cell is
 * the first maximal cell in row-major order (query rows outer); the walk back from H prefers the diagonal, then E, then F; inside
 * E (F) the gap opens at this cell when E[i][j] = H[i][j-1] - open - ext, else extends; it stops at H = 0.  Coordinates are
 * 1-based, length = columns, gapopen = gap runs, pident = 100 identical / length as %.2f (identity of the codes).
 * Device (csrc/sw.hip): one lane group per (query, chunk of one genome's subjects), each lane a strip of T query rows in
 * registers, the chunk's subjects streaming through the lanes back to back as a systolic anti-diagonal pipeline; classes by
 * query length with groups of 16 / 32 / 64 lanes (pml_sw_class_limits), the widest in passes over a line buffer.  The winner
 * per (query, genome) is kept on the device as a 64-bit key (S << 32 | 0xFFFFFFFF - position) under a global integer maximum:
 * the nq x G keys are the only download. */
typedef struct pml_sw_opts {
    int gap_open, gap_extend;                         /* 0 = 11, 1 */
    double lambda, K, evalue;                         /* 0 = 0.267, 0.041, 0.1 */
    int hits_per_query, traceback;                    /* 0 or 1; 0 or 1 */
    const int *table576;                              /* NULL = BLOSUM62 as loaded */
} pml_sw_opts;
typedef struct pml_proteome_set {
    int ngenomes;
    const int *genome_off;                            /* [ngenomes + 1] into labels / residues */
    const char *const *labels;
    const char *const *residues;                      /* NUL-terminated */
} pml_proteome_set;
typedef struct pml_sw_result {
    long long nhits;
    int *query, *subject;                             /* [nhits] global protein indices */
    int *target_genome, *score;
    double *bits, *evalue;
    char *table; long long table_bytes;               /* the table text */
    long long cells;                                  /* DP cells of the search: the sum of m n over all pairs */
} pml_sw_result;
int  pml_sw_search(pml_ctx *ctx, const pml_proteome_set *set, const pml_sw_opts *opts, pml_sw_result *result);
/* the same rule in plain C++ loops, no context (csrc/sw_host.cpp): the CPU tests' subject and the timing baseline */
int  pml_sw_search_host(const pml_proteome_set *set, const pml_sw_opts *opts, pml_sw_result *result);
void pml_sw_result_free(pml_sw_result *result);
/* limits_out[8] = per class lanes and the longest query of one pass (16 T, 32 T, 64 T; the last class takes longer ones in
 * passes), then the strip T and the default chunk's stream bytes */
int  pml_sw_class_limits(int *limits_out);
/* test door: the raw score of every pair, no selection.  The subjects are treated as one genome (chunks and units as in a
 * search).  force_class -1 = by length, 0 .. 2 = that class (PML_EINVAL when a query is longer than the class's one pass and
 * the class is not the last); force_path 0 = int32, the only path built */
int  pml_debug_sw_scores(pml_ctx *ctx, int nq, const char *const *queries, int ns, const char *const *subjects, const pml_sw_opts *opts,
                         int force_class, int force_path, int *scores_out /* [nq][ns] */);
/* launches[4] = k_sw_score launches per class and work units on this context so far, *cells the DP cells they covered; with
 * cfg.profile = 1 total_ms[4] = the three classes and the uploads (HIP events).  Never reset. */
int  pml_sw_stats(pml_ctx *ctx, long long *launches, long long *cells, double *total_ms);

/* ---- Multiple alignment: progressive profile alignment of the selected sets ----
 * The step between pml_homolog_groups' set_<k>.faa files and everything that starts from aligned genes.  The reference does it in
 * PhylogenomicPipeline2.alignAll (:701-725) and getAlignment (:737-806) through MultipleSequenceAligner.getMSA (:90-141), which
 * runs `muscle -fasta -stable -quiet`, and getProfileMSA (:143-218), which runs `muscle -profile -in1 -in2`.  muscle is in the
 * reference as a binary without source, so PARITY WITH muscle IS UNPINNED: the alignment is rebuilt from the rule below, in exact
 * integers on the device, in the host twin (csrc/msa_host.cpp) and in tests/msa_ref.py.
 * Input: a set is n >= 1 proteins in the caller's order.  Residues are encoded as the homology search encodes them (23 codes,
 * J O U -> X); any other byte is PML_EINVAL naming sequence and position, and so is a sequence of length 0.  table576 (NULL =
 * BLOSUM62 as loaded) must fit int8 and need not be symmetric; gap_open / gap_extend 0 = 11 / 1.
 * Guide tree: S(a, b), a < b, is the homology search's Smith-Waterman score of a as the query against b as the subject (same
 * table and costs; k_sw_score on the device, sw_score_host in the twin).  Clusters start as single sequences; a cluster's id is
 * its lowest member index.  Until one cluster remains the pair of clusters with the largest average of S over its cross pairs is
 * merged; two averages are compared exactly (Sum_AB |C||D| against Sum_CD |A||B| in 128-bit integers), ties go to the lowest
 * first id, then the lowest second id.  In a merge the cluster with the lower id is X, the other Y; the merged rows are X's rows,
 * then Y's rows.  A merge's level is 1 + the larger level of its two clusters, single sequences 0.
 * Profile alignment of X (nX rows, LX columns) and Y (nY rows, LY columns): w = nX nY, GO = gap_open w, GE = gap_extend w,
 * s(i, j) = Sum_a Sum_b cX[i][a] cY[j][b] T[a][b] over the 23 codes, cX[i][a] the rows of X with code a in column i (gap cells add
 * nothing).  A gap run before the first or behind the last column of the other profile pays no open cost: oE(i) = 0 for i in
 * {0, LX}, else GO; oF(j) = 0 for j in {0, LY}, else GO.
 *   H[0][0] = 0
 *   E[i][j] = max(E[i][j-1] - GE, H[i][j-1] - oE(i) - GE)     j >= 1   (a column of Y against gaps in X)
 *   F[i][j] = max(F[i-1][j] - GE, H[i-1][j] - oF(j) - GE)     i >= 1   (a column of X against gaps in Y)
 *   H[i][j] = max(H[i-1][j-1] + s(i, j), E[i][j], F[i][j])             terms that do not exist are minus infinity
 *   score   = H[LX][LY]
 * Traceback from (LX, LY): in H the diagonal is preferred, then E, then F; inside E the run opens at this cell when
 * E[i][j] = H[i][j-1] - oE(i) - GE, else it extends; F likewise.
 * Cells are int32.  A merge is refused (PML_EINVAL naming the set and the bound) when
 *   w ((M + gap_open) (min(LX, LY) + 1) + gap_extend (LX + LY)) >= 2^30,   M the largest |table entry|,
 * checked on the host with the two profiles' actual lengths before the merge is launched; an int64 path is not built.  Minus
 * infinity is -2^30.  Only E[i][0] and F[0][j] hold it.  Every other cell is the score of a real path: it is at most w M min(LX,
 * LY) and at least -(GE (LX + LY) + 2 GO), both inside the bound, so it is above -2^30, and minus infinity less one GE (the most
 * it is lowered by before a real term replaces it) never wins or ties a maximum and stays above -2^31.
 * The counts and V_j[a] = Sum_b cY[j][b] T[a][b] are int16 on the device: a merge with nX > 32767 or nY > 255 is PML_EINVAL (no
 * int32 count path is built).
 * Output (-stable): the rows in input order, all of one length, `-` for a gap, residues as encoded (upper case, J O U as X).  A set
 * of one sequence is that sequence.
 * NOT BUILT: muscle's k-mer distances, its second (Kimura) tree, refinement by tree bipartitioning, its log-expectation score and
 * position-specific gap costs, anchors and diagonals, Hirschberg or any linear-space mode.
 * Device (csrc/msa.hip): the pair scores come from the homology search's driver, consecutive sets sharing a call until they hold 96
 * sequences.  All merges of one level of all sets of a call go through one round of launches: k_msa_colv (V_j of every
 * Y), k_msa_dp (lane groups of 16 / 32 / 64 lanes by LX, a lane a strip of T = 8 columns of X in registers, Y's columns
 * streaming through the lanes; one direction word per strip and column: H source, E opened, F opened, four bits a cell),
 * k_msa_walk (the traceback, one lane per merge, writes the merged column map) and k_msa_gather (the merged rows and counts).
 * Between levels only the merged lengths come back.  The direction words live in an HBM scratch; a level is cut into sub-batches
 * under the scratch budget (half the HBM budget, or PML_MSA_SCRATCH_BYTES), and a single merge above it is PML_ENOMEM. */
typedef struct pml_msa_opts {
    int gap_open, gap_extend;                         /* 0 = 11, 1 */
    const int *table576;                              /* NULL = BLOSUM62 as loaded */
} pml_msa_opts;
typedef struct pml_msa_set {
    int nseq;
    const char *const *residues;                      /* NUL-terminated; in a profile `-` is a gap */
} pml_msa_set;
typedef struct pml_msa_result {
    int nrows, ncols;
    char *rows;                                       /* nrows x (ncols + 1): every row NUL-terminated */
    int nmerges;                                      /* nrows - 1 (pml_msa_align), 1 (profile calls) */
    int *merge_x, *merge_y, *merge_level;             /* cluster ids in the order of the merges, and their levels */
    long long *merge_score;                           /* H[LX][LY] of every merge */
    unsigned char *path;                              /* profile calls: per merged column 0 = both, 1 = Y's column only, 2 = X's only; else NULL */
} pml_msa_result;
/* results[nsets].  On an error every result is empty. */
int  pml_msa_align(pml_ctx *ctx, int nsets, const pml_msa_set *sets, const pml_msa_opts *opts, pml_msa_result *results);
/* the same rule in plain C++ loops, no context (csrc/msa_host.cpp): the CPU tests' subject and the timing baseline.  err (may
 * be NULL) receives the message of a failure, at most err_cap bytes with the NUL */
int  pml_msa_align_host(int nsets, const pml_msa_set *sets, const pml_msa_opts *opts, pml_msa_result *results, char *err, int err_cap);
/* two given alignments (getProfileMSA): a is X, b is Y; rows of equal length, `-` a gap.  The merged rows are a's, then b's */
int  pml_msa_profile_align(pml_ctx *ctx, const pml_msa_set *a, const pml_msa_set *b, const pml_msa_opts *opts, long long *score_out, pml_msa_result *result);
int  pml_msa_profile_align_host(const pml_msa_set *a, const pml_msa_set *b, const pml_msa_opts *opts, long long *score_out, pml_msa_result *result,
                                char *err, int err_cap);
/* the merges of a set of n sequences from its pair scores (scores[a * n + b], a < b, is read): n - 1 merges */
int  pml_msa_guide_tree_host(int n, const long long *scores, int *merge_x, int *merge_y, int *merge_level);
void pml_msa_result_free(pml_msa_result *result);
/* limits_out[8] = per class lanes and the columns of X of one pass (16 T, 32 T, 64 T; the last class takes longer ones in
 * passes over a line buffer), then the strip T and the threads of a workgroup */
int  pml_msa_limits(int *limits_out);
/* test door: pml_msa_profile_align with the class forced (-1 = by LX; PML_EINVAL when X is longer than the class's one pass and
 * the class is not the last) */
int  pml_debug_msa_profile_align(pml_ctx *ctx, const pml_msa_set *a, const pml_msa_set *b, const pml_msa_opts *opts, int force_class, long long *score_out,
                                 pml_msa_result *result);
/* counts[8] = k_msa_colv, k_msa_dp, k_msa_walk, k_msa_gather launches, merges, levels, sub-batches and DP cells on this context
 * so far; with cfg.profile = 1 total_ms[4] = the four kernels (HIP events).  Never reset. */
int  pml_msa_stats(pml_ctx *ctx, long long *counts, double *total_ms);

/* Concurrent pml_score / pml_optimize / pml_search calls on one context (PEPR's tree_threads workers) are
 * coalesced into device batches; this reports how many batches ran and how many single calls they carried. */
int pml_coalescing_stats(pml_ctx *ctx, long long *batches, long long *requests);

/* The branch-length Newton kernel splits a request over several workgroups that exchange partial sums.  Its forward progress
 * does not depend on dispatch order (slices are claimed by ticket), and its waits are bounded in wall-clock time: when a wait
 * gives up (a co-tenant of the GPU kept a request's slices apart for > 2 s), the affected requests -- in a chained smoothing
 * pass, the whole pass -- are re-issued through a no-exchange form of the same kernel whose results are bit-identical, and the
 * call succeeds.  This reports how often that happened on the context: give-up events, requests re-issued, launches of the
 * no-exchange form (all 0 on a GPU the process has to itself). */
int pml_newton_fallbacks(pml_ctx *ctx, long long *giveups, long long *reissued, long long *seq_launches);

/* Every computing entry point runs its host-side arithmetic under the DEFAULT floating-point control state (round to
 * nearest, no flush-to-zero / denormals-are-zero) whatever the calling thread -- a JVM worker, a Python thread -- came in
 * with, and restores the caller's state on return: results do not depend on the caller's MXCSR.  Diagnostic: the distinct
 * control states callers entered with (returns their number; values[] receives up to cap of them). */
int pml_debug_fpenv(unsigned *values, int cap);

/* profiling: HIP-event time of device kernels since the last reset (cfg.profile = 1) */
enum { PML_K_PMAT = 0, PML_K_NEWVIEW = 1, PML_K_EVALUATE = 2, PML_K_SUMTABLE = 3, PML_K_NEWTON = 4,
       PML_K_REDUCE = 5,
       PML_K_HOST_BUILD = 6 /* CPU ms building descriptors */, PML_K_HOST_WAIT = 7 /* CPU ms in stream sync */,
       PML_K_MODEL = 8 /* model builds (k_model): eigen-systems of per-gene and registered rate matrices */, 
       PML_K_CODEHIST = 9 /* code histograms of device-gathered replicates (k_codehist); bytes = code-matrix bytes read */,
       PML_K_PAIRSCORE = 10 /* pair scores of the nj method (k_pairscore); bytes = code bytes read */,
       PML_K_COLSPLIT = 11 /* congruence filter: k_colsplits launches (count pass and write pass); bytes = alignment bytes read */,
       PML_K_SPLITCOST = 12 /* congruence filter: k_splitcost launches; bytes = split words read (distinct splits, and the kept set per workgroup) */,
       PML_K_COUNT = 13 };
/* slots added after PML_K_COUNT was published (a client that sizes an array by it keeps working); PML_K_END is one past the last */
enum { PML_K_TREEPAIRS = 13 /* tree-set comparison: k_tree_pairs launches (one per block of rows); bytes = 4 per set look-up */,
       PML_K_END = 14 };
int pml_kernel_stats(pml_ctx *ctx, int kernel, long long *launches, double *total_ms,
                     double *algo_bytes /* algorithmic bytes moved, SURVEY 8d figures */);
/* algorithmic flops of the launches counted by pml_kernel_stats, SURVEY 8d's per-operation figures (newview inner-inner 6480,
 * tip-inner 3280, tip-tip 80, evaluate 3360 flop per pattern; a sumtable = an inner-inner contraction) */
int pml_kernel_flops(pml_ctx *ctx, int kernel, double *algo_flops);
int pml_kernel_stats_reset(pml_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif
