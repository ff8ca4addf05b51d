// kernels.h -- device kernel interface of libpeprml (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "gblocks.hpp"
#include "mash.hpp"
#include "mcl.hpp"
#include "sw.hpp"
#include "treecmp.hpp"

namespace pml {

constexpr int NS = 20;                 // amino-acid states
constexpr int NCAT = 4;                // Gamma categories laid out per CLV (ncat=1 replicates)
constexpr int CLV_ROWS = NCAT * NS;    // 80 rows of `mpad` doubles: CLV[cat*20+state][pattern]
constexpr int PFRAG = NCAT * 25 * 16;      // doubles per transition-matrix fragment set (12.8 KB)
constexpr int PAT_PER_WAVE = 32;       // one MFMA chunk: 2 N-tiles of 16 patterns (16 B / lane)
// CLVs and sumtables are TILED in HBM: tile k holds patterns [128k, 128k+128) as 80 rows x 128 doubles = 80 KB contiguous,
// element (row, p) at ((p >> 7) * 80 + row) * 128 + (p & 127).  One k_oplist workgroup / one k_newton slice owns exactly one
// tile, so every CLV it reads or writes is ONE contiguous 80 KB stream (round 1: 80 separate 1 KB pieces 8 KB apart;
// profiles/r02_ubench_hbm.txt: contiguous tiles stream 5.9 TB/s for this 2R:1W mix, scattered 1 KB pieces 4.7-5.2).
constexpr int TILE_PAT = 128;
constexpr size_t clv_doubles(int mpad) { return (size_t)((mpad + TILE_PAT - 1) / TILE_PAT) * TILE_PAT * (NCAT * NS); }
constexpr size_t clv_index(int row, int p) { return ((size_t)(p >> 7) * (NCAT * NS) + (size_t)row) * TILE_PAT + (size_t)(p & (TILE_PAT - 1)); }
constexpr int NCODES = 23;
// tip table: T[c][code][q][kk] (kk padded to 6) = sum_{j in code} P_c[s = 4 kk + q][j]: the five rows a lane
// needs (its q, kk = 0..4) are 40 contiguous bytes of a 48-byte, 16-byte-aligned record -> 3 loads instead of 5
// gathers (17.7 KB per branch)
constexpr int TIPTAB_KK = 6;
constexpr int TIPTAB_DOUBLES = NCAT * NCODES * 4 * TIPTAB_KK;
constexpr int FRAG_STRIDE = TIPTAB_DOUBLES;          // doubles per k_pmat output slot (fragment set or tip table)

// device-resident model constants (one per ctx)
struct ModelDev {
    double eval[NS];
    double U[NS * NS];      // row-major U[s][k]
    double Uinv[NS * NS];   // Uinv[k][j]
    double pi[NS];
    double UinvT[NS * NS];  // UinvT[j][k] = Uinv[k][j]: a column of Uinv contiguous (k_pmat reads it with scalar loads)
};

// request for one model build (k_model): the eigen-system of the reversible rate matrix with exchangeabilities `exch` (190,
// lower triangle by rows, state order ARNDCQEGHILKMFPSTWYV) and frequencies `pi` (20, normalised by the kernel), both in HBM.
// patch >= 0: entry `patch` of exch counts as patch_val and memory is not touched -- one trial value of one rate while the
// exchangeabilities are being estimated (PROTGAMMAGTR)
struct ModelReq {
    const double *exch;
    const double *pi;
    ModelDev *out;
    int patch;
    double patch_val;
};
constexpr int NEXCH = NS * (NS - 1) / 2;

// request for one transition-matrix fragment set: P(t * rate_c), c = 0..3
struct PmatReq {
    double t;
    double rates[NCAT];
    int kind;               // PM_FRAGS, PM_FRAGS_PI (rows scaled by pi_s: root evaluation), PM_TIPTABLE
    int pad;
    const double *tp;       // non-null: the length is read from device memory (written by an earlier k_newton of
                            // the same stream: chained smoothing pass), `t` is ignored
    const ModelDev *md;     // per-gene model (PROTGAMMAWAGF: empirical frequencies); null = the launch's model
};
enum { PM_FRAGS = 0, PM_FRAGS_PI = 1, PM_TIPTABLE = 2 };

// one side (child) of a CLV operation
//   SK_CLV    : p0 = CLV (80 x mpad doubles) in HBM
//   SK_TIP    : p0 = tip codes (uint8[mpad]); t0 = tip table of its branch (newview only)
//   SK_CHERRY : the child is an inner node whose two other neighbours are tips.  Its CLV is never
//               materialised: operand[c][s] = T0[c][code0][s] * T1[c][code1][s] from the two tip
//               tables (p0/p1 = codes of the two tips, t0/t1 = their tables), then contracted with
//               the fragment set of the branch to the parent like any CLV.
//   SK_PITCH  : the child X is an inner node over a cherry C (tips a,b) and a tip c ("pitchfork", 3 tips):
//               CLV_X[c][s] = (P(t_XC) . (T_a * T_b))[s] * T_c[s] is rebuilt in registers (one extra
//               contraction with the fragment set `f` of branch X-C) and then used like a CLV.
//               p0,p1,p2 = codes of a,b,c; t0,t1,t2 = their tip tables.
enum { SK_CLV = 0, SK_TIP = 1, SK_CHERRY = 2, SK_PITCH = 3 };
constexpr int OPF_NT_STORE = 16;
// Register chaining (k_oplist<9>): a wave owns the same 32 patterns in every operation of its gene, so the result of one
// newview is still in its registers when the next operation of the gene consumes it (post-order: a parent directly follows
// its last-computed child).  OPF_CHAIN_L / OPF_CHAIN_R: that side (kind SK_CLV) is taken from the registers instead of being
// read back; OPF_NO_STORE: the result is consumed that way only and is not written at all (whole-tree scoring).
// OPF_CHAIN_R is honoured on MODE_EVALUATE* operations only (a newview's chained child always goes left, engine.cpp); a
// MODE_SUMTABLE operation leaves its own tile in those registers, so nothing is chained from across one.
constexpr int OPF_CHAIN_L = 32, OPF_CHAIN_R = 64, OPF_NO_STORE = 128;
// Fused branch Newton (k_oplist<11>, round 3): a MODE_SUMTABLE operation that is the LAST operation of its gene in the launch
// does not store its table -- a workgroup's tile of it (128 patterns x 80 rows) stays in the 80 VGPRs per wave that register
// chaining reserves, and the gene's workgroups run makenewz on it in place (one exchange of three sums per evaluation, as in
// k_newton).  Saves the sumtable's write and read (2 of the 5 CLV-sized transfers of a smoothing step), k_newton's launch and ramp.
constexpr int OPF_FUSED_NEWTON = 256;
struct OpSide {
    const void *p0, *p1, *p2;
    const double *t0, *t1, *t2;
    const double *f;
};

// one CLV operation (newview / sumtable / evaluate share the descriptor)
struct NvOp {
    double *out;            // newview: CLV; sumtable: table; evaluate: per-pattern lnL
    OpSide l, r;
    int *out_scl;           // per-pattern scaling counts of the result (may be null for evaluate)
    const int *l_scl;       // null unless the side is SK_CLV
    const int *r_scl;
    const double *pl;       // fragment sets (PFRAG doubles); null for a newview SK_TIP side
    const double *pr;
    int mpad;               // padded pattern count (multiple of 32)
    int flags;              // bits 0-1: left side kind, bits 2-3: right side kind, OPF_*
    int mode;               // MODE_NEWVIEW / MODE_SUMTABLE / MODE_EVALUATE
    int pad;
    const void *aux;        // OPF_FUSED_NEWTON sumtable ops: the NewtonReq (device address) the workgroups of the gene iterate on, else null
};
static_assert(sizeof(NvOp) == 184, "NvOp layout");

// ops [op_begin, op_end) of one gene, in dependency order; executed by every pattern block
struct GeneRun {
    int op_begin, op_end;
};

struct ReduceReq {          // lnL_g = sum_p w[p] * patlnl[p]
    const double *patlnl;
    const double *weight;
    double *out;
    int mpad;
    int pad;
};

struct NewtonReq {          // Newton-Raphson on one branch from its sumtable
    const double *sumtab;   // [80][mpad]
    const double *weight;   // [mpad]
    const int *scl;         // [mpad] combined scaling counts
    double rates[NCAT];
    double t0;
    double tol;             // stop when |dt| < tol
    double *out;            // out[0]=t, out[1]=lnL, out[2]=d1, out[3]=d2 (at returned t)
    double *sync;           // NEWTON_SYNC_DOUBLES 8-byte words: the slices' {tag, value} exchange granules; never cleared: tags are unique
    const ModelDev *md;     // eigenvalues of the gene's model
    unsigned tag_base;      // (launch number << 10): granule tag = tag_base + evaluation number, so a block left by an earlier launch never matches
    unsigned pad0;
    double *t_dev0, *t_dev1; // optional: device-resident copies of the branch length (both directions) for chaining
    double *patlnl;         // optional: per-pattern lnL (scaling applied) at the returned length, [mpad] (SH-like supports)
    int mpad;
    int max_iter;           // 0: derivatives at t0 only
    int ticket0;            // first ticket of this request in its kernel's ticket table (k_newton: slice = ticket - ticket0)
    int pad;
};
constexpr int NEWTON_MAX_SPLIT = 64;    // 128-pattern slices up to 8192 patterns stay register-resident (k_newton)
// the split of a request over workgroups: a function of its pattern count alone (bit-reproducible whatever shares the launch)
constexpr int NEWTON_SLICE_PAT = 128;
__host__ __device__ constexpr int newton_split(int mpad) { return (mpad + NEWTON_SLICE_PAT - 1) / NEWTON_SLICE_PAT < NEWTON_MAX_SPLIT ? ((mpad + NEWTON_SLICE_PAT - 1) / NEWTON_SLICE_PAT < 1 ? 1 : (mpad + NEWTON_SLICE_PAT - 1) / NEWTON_SLICE_PAT) : NEWTON_MAX_SPLIT; }
// register form: a slice IS a tile of the sumtable (80 KB contiguous); beyond 64 tiles the slices grow and stream
__host__ __device__ constexpr int newton_slice(int mpad) { return mpad <= NEWTON_SLICE_PAT * NEWTON_MAX_SPLIT ? NEWTON_SLICE_PAT : ((mpad / 32 + newton_split(mpad) - 1) / newton_split(mpad)) * 32; }
__host__ __device__ constexpr bool newton_reg_form(int mpad) { return newton_slice(mpad) <= NEWTON_SLICE_PAT; }
// per (batch, stream) control block of k_newton, zeroed once at allocation: ticket / done counters of the register-form [0]
// and streaming-form [1] kernels (the last workgroup of a launch re-arms them) and the sticky abort word the host clears
// oticket / odone: k_oplist launches with fused Newton tails claim (gene, tile) by ticket as well, one counter per XCD partition
// dbg: what the first slice that gave up saw (diagnostic, printed under PML_TRACE): {1, slice, S, evaluation, mask of slices
// whose granules had arrived (low / high 32), tag wanted, 0}
struct NewtonCtl { int ticket[2]; int done[2]; int abort; int odone; int pad[2]; int oticket[8]; int dbg[8];
                   unsigned long long n_requests, n_evals; };     // diagnostic totals (PML_TRACE): Newton requests served, evaluations made
constexpr int NEWTON_SYNC_DOUBLES = 2 * NEWTON_MAX_SPLIT * 6;   // two parities x slices x six 8-byte {tag, half a double} granules (three partial sums)

// MODE_EVALUATE_CAT: like MODE_EVALUATE but the four categories are NOT averaged: out[c][p] = sum_s L_c[s] (pi P_c . R_c)[s]
// (plain likelihoods, 4 x mpad doubles) and out_scl[p] = the pattern's scaling count -- the per-site x rate likelihood
// table of FastTree's Gamma20 re-weighting, four rates per traversal
enum { MODE_NEWVIEW = 0, MODE_SUMTABLE = 1, MODE_EVALUATE = 2, MODE_EVALUATE_CAT = 3 };

// FastTree -gamma (FastTreeRunner.java:67-70): lnL of one gene under 20 FIXED rates with category weights w[k]:
//   lnL = sum_p weight[p] * ( ln( sum_k w[k] * table[k][p] * 2^(-256 (cnt[k/4][p] - m_p)) ) - m_p * 256 ln 2 ),  m_p = min_j cnt[j][p]
constexpr int G20_RATES = 20;
struct G20Req {
    const double *table;    // [20][mpad] per-pattern likelihoods, rate k in row k (five MODE_EVALUATE_CAT traversals)
    const int *cnt;         // [5][mpad] scaling counts of the five traversals
    const double *weight;   // [mpad] pattern weights
    double w[G20_RATES];    // category weights
    double *out;            // lnL
    double *patlnl;         // optional [mpad]
    int mpad, pad;
};
void launch_g20(const G20Req *reqs, int n, hipStream_t s);

// one gene's patterns copied into a replicate (jackknife concatenation on the device):
// dst[t][dst_off + p] = rowmap[t] >= 0 ? src[rowmap[t]][p] : gap code, dst_w[dst_off + p] = w[p]
struct GatherSeg {
    const uint8_t *src; const double *w; uint8_t *dst; double *dst_w; const int *rowmap;
    int src_mpad, npat, dst_mpad, dst_off, ntax_dst, pad;
};
void launch_gather(const GatherSeg *segs, int nsegs, int max_npat, hipStream_t s);
// freq.hip k_codehist: out[r][code] += the summed weights (integers stored as f64) of the cells of replicate r's code matrix
// that hold `code`; one launch for all replicates, `out` (nreqs x NCODES, 64-bit integers) zeroed by the caller
struct CodeHistReq { const uint8_t *codes; const double *weight; int ntax, mpad; };
void launch_codehist(const CodeHistReq *reqs, int nreqs, int max_mpad, long long *out, hipStream_t s);
// pairscore.hip k_pairscore: out[i][j] += sum_k table[codes[i][k]][codes[j][k]] over the sites of the request's gene, every
// ORDERED taxon pair (the table may be asymmetric); one launch for all requests.  codes: ntax rows of ld bytes (ld a multiple
// of 16, the array 16-byte aligned, every byte < PS_CODES); out: ntax x ntax 64-bit integers zeroed by the caller on the
// same stream.  table: PS_CODES x PS_TSTRIDE int8 in device memory.  chunk_sites: sites per workgroup, a multiple of 16,
// <= PS_MAX_CHUNK (the int32 accumulator of a pair holds a whole chunk)
constexpr int PS_CODES = 24, PS_TSTRIDE = 32, PS_TILE = 16, PS_STAGE = 512, PS_MAX_CHUNK = 1 << 20, PS_CHUNK_DEFAULT = 2048;
struct PairScoreReq { const uint8_t *codes; long long *out; int ntax, nsites, ld; };
void launch_pairscore(const PairScoreReq *reqs, int nreqs, int max_ntax, int max_nsites, int chunk_sites, const int8_t *table, hipStream_t s);
// pairscore.hip k_pairscore_sum: out[i][j] = sum over the nsel selected genes g of S_g[loc_g(i)][loc_g(j)] for the nu x nu pairs
// of a replicate's taxon union; loc (nsel rows of nu ints, -1 = the gene lacks the taxon: contributes 0) and sel index the
// call-wide arrays S (per-gene matrices) and gene_ntax
struct PairSumReq { const int *sel; const int *loc; long long *out; int nsel, nu; };
void launch_pairscore_sum(const PairSumReq *reqs, int nreqs, int max_nu, const long long *const *S, const int *gene_ntax, hipStream_t s);

// The congruence filter (congruence.hip): the splits of every alignment column as records of W 64-bit words over the n taxa of
// the concatenation (taxon i = bit i & 63 of word i >> 6; W = 1, 2, 4 or 8, the smallest that holds n <= CG_MAX_TAXA bits).
// A gene's rows are raw bytes, ld bytes apart (a multiple of 16, the array 16-byte aligned), in ASCENDING order of their union
// index; map[r] = union index of row r.  A taxon the gene lacks has no row and sets no bit.
constexpr int CG_MAX_TAXA = 512, CG_COLS = 64 /* columns per k_colsplits workgroup */, CG_KTILE = 256 /* kept splits per LDS tile of k_splitcost */;
constexpr int cg_words(int n) { return n <= 64 ? 1 : n <= 128 ? 2 : n <= 256 ? 4 : 8; }
struct CgGene { const uint8_t *bytes; const uint16_t *map; int ntax, ncols, ld; long long col_base; /* index of its first column in the call */ };
// one workgroup per entry of tile_gene (gene index; a gene's tiles are consecutive, tile_first[gene] = its first); max_ntax sizes the LDS.
// count pass (rec == nullptr): nsplit[column] = the column's number of splits.  write pass: rec_off[column] = exclusive
// prefix of nsplit; record rec_off[column] + i = the column's i-th split in ascending order of the class's byte, normalised;
// rec_gene / rec_col = its gene and its column index in the call
void launch_colsplits(const CgGene *genes, const int *tile_gene, const int *tile_first, int ntiles, int max_ntax, int n, int *nsplit,
                      const long long *rec_off, unsigned long long *rec, int *rec_gene, long long *rec_col, hipStream_t s);
// interning: slot[cap] (cap a power of two, filled with -1 by the caller) holds the index of the first record of its key;
// split_id[r] = that owner's index; count[owner] += 1 for every record of at least 2 members (zeroed by the caller).
// hash_mask is ANDed onto the hash before it is reduced to a slot.  *err is set when a probe runs through the whole table
void launch_split_intern(const unsigned long long *rec, long long nrec, int W, int *slot, unsigned long long cap, unsigned long long hash_mask,
                         int *split_id, int *count, int *err, hipStream_t s);
// out[j][W] = rec[idx[j]][W]
void launch_split_gather(const unsigned long long *rec, const int *idx, long long nidx, int W, unsigned long long *out, hipStream_t s);
// cost_d[d] = cost_rec[dist[d]] = sum of kcount[j] over the kept splits kwords[j] that conflict with record dist[d]
void launch_splitcost(const unsigned long long *rec, const int *dist, long long ndist, int W, const unsigned long long *kwords, const int *kcount,
                      long long nkept, long long *cost_d, long long *cost_rec, hipStream_t s);
// per gene: the distinct split ids of its records (second table: keys[cap] filled with ~0 by the caller), cost_sum[gene] +=
// cost_rec[id] and ndistinct[gene] += 1 once per distinct (gene, id)
void launch_genecost(const int *rec_gene, const int *split_id, long long nrec, const long long *cost_rec, unsigned long long *keys,
                     unsigned long long cap, unsigned long long hash_mask, long long *cost_sum, int *ndistinct, int *err, hipStream_t s);

// Column trimming (trim.hip, rules in trim.hpp): MSATrimmer's three filters in front of the congruence filter.  Genes come in
// the CgGene layout (map is not read; ntax = the gene's own rows, any number of them).
// k_colclass: one workgroup per entry of tile_gene (TRIM_COLS columns of that gene, tile_first[gene] = its first tile), thread =
// one column: flags[col_base + column] = the column's TRIM_* byte; gap_or_missing[gene] += its '-' and '?' cells (zeroed by the caller)
void launch_colclass(const CgGene *genes, const int *tile_gene, const int *tile_first, int ntiles, uint8_t *flags, long long *gap_or_missing, hipStream_t s);
// k_colgather: out[r][j] = in[r][src_col[j]] for j < nkept, 0 for nkept <= j < ld_out; ld_out = nkept rounded up to 16, src_col holds
// ld_out entries (16-byte aligned, the padding ones anything), out is 16-byte aligned.  One workgroup per tile: TRIM_CHUNKS
// 16-byte chunks of TRIM_ROWS rows of one gene, from chunk0 and row0
struct TgGene { const uint8_t *in; uint8_t *out; const int *src_col; int ntax, nkept, ld_in, ld_out; };
struct TgTile { int gene, chunk0, row0, pad; };
void launch_colgather(const TgGene *genes, const TgTile *tiles, int ntiles, hipStream_t s);

// Block trimming (gblocks.hip, rules in gblocks.hpp): the reference's `-gblocks_trim`.  Genes in the CgGene layout as above, plus
// one GbGene each: the resolved parameters, src_col (ld ints, 16-byte aligned) and, for a gene of more than GB_LDS_COLS columns,
// scratch (2 * ncols ints).
// k_gbclass: tiles as k_colclass; flags[col_base + column] = gb_class's byte, gap_or_missing[gene] += its '-' and '?' cells
// k_gbselect: one workgroup per gene: the five rounds on flags[col_base ..] (stage bits ORed in), then the kept columns' indices,
// ascending, to src_col (the entries up to the next multiple of 16: -1) and their number to tg[gene].nkept, rounded up to 16 to
// tg[gene].ld_out -- what k_colgather reads, so that it can follow without the host in between
struct GbGene { int ntax, ncols; long long col_base; int *src_col; int *scratch; GbParams p; };
void launch_gbclass(const CgGene *genes, const GbGene *gb, const int *tile_gene, const int *tile_first, int ntiles, uint8_t *flags,
                    long long *gap_or_missing, hipStream_t s);
void launch_gbselect(const GbGene *gb, int ngenes, uint8_t *flags, TgGene *tg, hipStream_t s);

// The gene homoplasy test (genesteps.hip; rules in include/peprml.h, draw functions in genesteps.hpp).  A sub-batch's genes: raw
// bytes in the CgGene layout (rows ld bytes apart) for k_colminsteps, site2pat for k_steps_expand; pat_off = the gene's first
// pattern in the replicate of all genes of the sub-batch, col_base = its first column in the sub-batch's steps / min_steps.
constexpr int GS_COLS = 256;          // columns per k_steps_expand / k_colminsteps workgroup, one per thread
enum { GS_RAW = 0, GS_BEYOND = 1, GS_RATIO = 2 };
struct GsGene { const uint8_t *bytes; const int *site2pat; int ntax, ncols, ld, pat_off; long long col_base; };
// one Fitch operation on vectors of the pool ([vector][mpad]): a union of l and r counts one step; out >= 0: out = F(l, r)
struct GsOp { int out, l, r, pad; };
// pat_steps[p] = the unions pattern p takes over the nops operations, p < npat <= mpad
void launch_fitch_sitesteps(const GsOp *ops, int nops, unsigned *pool, int mpad, int npat, int *pat_steps, hipStream_t s);
// one workgroup per entry of tile_gene (GS_COLS columns of that gene, tile_first[gene] = its first tile), as launch_colclass
void launch_steps_expand(const GsGene *genes, const int *tile_gene, const int *tile_first, int ntiles, const int *pat_steps, int *steps, hipStream_t s);
// min_steps[col_base + column] = classes - 1 - [classes == 2 and shown == n_union]; -1: the column holds only '-' and '?'
void launch_colminsteps(const GsGene *genes, const int *tile_gene, const int *tile_first, int ntiles, int n_union, int *min_steps, hipStream_t s);
// table[i] = steps[i] (GS_RAW), steps[i] - mins[i] (GS_BEYOND), both int, or (float)steps[i] / (float)(mins[i] + 1) (GS_RATIO, float)
void launch_steps_table(const int *steps, const int *mins, long long n, int statistic, void *table, hipStream_t s);
// one gene of a resampling launch: len draws per replicate from a domain of U table indices; a domain index u reads table[u]
// below split and table[u + len] from it on (a masked gene: split = U).  sums[entry * reps + b], int or float as the table
struct GsEntry { int gene; uint32_t len, U, split; };
void launch_steps_resample(const GsEntry *entries, int nentries, const void *table, void *sums, int reps, unsigned long long base, bool as_float, bool replace,
                           hipStream_t s);

// Tree-set comparison (treecmp.hip): the split records of T trees, compact: tree t owns entries off[t] .. off[t] + cnt[t] - 1 of
// every array, its first nreal[t] are TreeBranches in the Java's order (treecmp.hpp).  id = interned split id, ln / lr =
// length over the tree's maximum / the length itself, flags = TC_*; sid / sidx = the tree's (id, record index) pairs sorted
// by id, for equal ids the highest index last (written by launch_tree_sort, which also sets TC_LAST).
constexpr int TC_COLS = 256 /* column trees per k_tree_pairs workgroup, one per lane */, TC_SORT = 2048 /* keys k_tree_sort sorts in LDS: cnt[t] <= TC_SORT */;
static_assert(3 * TC_MAX_TAXA <= TC_SORT && TC_MAX_TAXA == CG_MAX_TAXA && tc_words(200) == cg_words(200), "a tree has fewer than 3 n records");
struct TcTrees { const int *off, *cnt, *nreal; int *id, *flags; const double *ln, *lr; int *sid, *sidx; int T; };
// id[r] (the owner launch_split_intern gave) becomes the index of the FIRST record of its split; first[nrec] filled with 0x7F bytes by the caller
void launch_tree_first(int *id, long long nrec, int *first, hipStream_t s);
// sorts every tree's ids, sets TC_LAST, then ss[t] = {sum ln^2, sum lr^2} over the tree's branches in order and
// distinct[t] = {distinct splits, distinct non-trivial splits} among them
void launch_tree_sort(const TcTrees &t, double *ss, int *distinct, hipStream_t s);
// rows i0 .. i0 + nrows - 1 against every column j >= i (window > 0: j - i <= window): counts[row * T + j] = {shared splits,
// shared non-trivial splits, shared splits of the resolved trees (rf_splits), 0}, sums[row * T + j] = {r of getBranchDistance,
// r of getDiscrepantBranchDistance}; other entries are not written.  maxrec >= every cnt[t] sizes the LDS (tree_pairs_lds)
size_t tree_pairs_lds(int maxrec);
void launch_tree_pairs(const TcTrees &t, int i0, int nrows, int window, int maxrec, int4 *counts, double2 *sums, hipStream_t s);

// SH-like local support of one split (FastTree's SHSupport; Guindon et al. 2010): per-pattern lnL of the current
// arrangement (l0) and of its two NNI alternatives (l1, l2); nboot resamples of nsites alignment columns drawn with
// the counter hash col(r, j) = mix64((seed+1)*0x9E3779B97F4A7C15 + r*nsites + j) % nsites; a resample supports the
// split when the centred advantage of its best arrangement is smaller than the observed advantage of l0
struct ShReq { const double *l0, *l1, *l2; const int *site2pat; double *out; unsigned long long seed; int nsites, nboot; };
void launch_sh(const ShReq *reqs, int n, hipStream_t s);
#ifdef __HIPCC__
// the counter hash of every device-side resampler (k_sh, k_rell): splitmix64's finaliser
__device__ __forceinline__ unsigned long long mix64(unsigned long long z) {
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull; z ^= z >> 27; z *= 0x94D049BB133111EBull; z ^= z >> 31;
    return z;
}
#endif

// Tree selection tests (CONSEL's makermt | consel | catpv, TreeComparison.java:812-885): multiscale RELL resampling of a
// per-site lnL table and the bootstrap / KH / SH counts of every tree, one launch (rell.hip).
//   table   X[N][tpad], site-major f64 in HBM (tpad = T rounded up to even: 16-byte rows), built by launch_rell_pack
//   draws   replicate b of scale k draws n_k sites: site_j = ((mix64(base + ((k B + b) << 32) + j) >> 32) * N) >> 32 with
//           base = (seed + 1) * 0x9E3779B97F4A7C15 (mod 2^64) -- no 64-bit division; a site's probability is off 1/N by at
//           most 2^-32 (absolute), i.e. by a factor within 1 +- N / 2^32
//   sums    Y[k][b][t] = sum_j X[site_j][t], plain f64 adds in ascending j in ONE thread's registers: a function of
//           (seed, k, b, N, X) alone, whatever the grid, the path or the rest of the launch
//   counts  (integer atomics: order-independent)  bp[k][t] += [t = argmax_t Y[k][b][t], lowest index of equals], every scale;
//           at scale k1 only, with L_t = sum_s X[s][t] in site order (launch_rell_pack) and C_t = Y_t * (N / n_k) - L_t:
//           sh[t] += [max_u C_u - C_t >= max_u L_u - L_t],   kh[t] += [C_u* - C_t >= L_u* - L_t], u* = argmax_{u != t} L_u
//           (lowest index of equals).  The replicates are centred on their EXACT expectation L_t, not on the replicate
//           mean CONSEL uses: one pass instead of two, and the two differ by O(B^-1/2) of a replicate's spread.
//   paths   lds = 1: every workgroup stages the table in dynamic LDS (rows padded to an odd number of 16-byte slots, so the
//           random b128 gathers spread over all 16 slots of a bank row) and gathers from there; lds = 0: gathers from
//           global memory (L2 / Infinity Cache).  Same bits.
struct RellReq {
    const double *X;                // [N][tpad]
    const double *L;                // [T] column sums in site order
    const int *ndraws;              // [K] n_k
    const double *scale;            // [K] N / n_k
    unsigned long long *bp;         // [K][T], zeroed by the caller
    unsigned long long *kh, *sh;    // [T]
    double *Y;                      // optional [K][B][T] (test door)
    unsigned long long base;        // (seed + 1) * 0x9E3779B97F4A7C15
    unsigned B;                     // replicates per scale
    int N, T, tpad, K, k1;
};
// The weighted tests (wKH, wSH) of the same replicates: the weighted arm of k_rell (launch_rell_weighted) counts bp / kh / sh
// exactly as the plain arm does and, at scale k1, from the same register sums
//   wsh[t] += [max_u (C_u - C_t) is_ut >= S_t],  S_t = max_u (L_u - L_t) is_ut,  u != t with is_ut > 0
//   wkh[t] += [(C_u* - C_t) is_u*t >= (L_u* - L_t) is_u*t],  u* = the u of S_t (lowest index of equals)
// with is_ut = 1 / sigma_ut from launch_rell_pairsd (0 = the pair is excluded).  Every ratio is one rounded multiply of a rounded
// difference.  A tree with no pair left counts every replicate.  The matrix is staged in dynamic LDS behind the table (LDS path)
// or alone (global path) and read with wave-uniform ds_read_b128.
struct RellWReq : RellReq {
    const double *isig;             // [tpad][tpad] 1 / sigma_ut, symmetric, 0 on the diagonal, for excluded pairs and the padding
    unsigned long long *wkh, *wsh;  // [T], zeroed by the caller
};
// rows of the LDS copy: tpad / 2 slots of 16 bytes rounded up to odd
constexpr int rell_lds_slots(int tpad) { return (tpad / 2) | 1; }
constexpr size_t rell_lds_bytes(int N, int tpad) { return (size_t)N * rell_lds_slots(tpad) * 16; }
// X[s][t] = src[t][site2pat ? site2pat[s] : s] (t < T; the padding column is 0), then L[t] = sum_s X[s][t] in site order
void launch_rell_pack(const double *const *src /* device array of T device pointers */, const int *site2pat, double *X, double *L,
                      int N, int T, int tpad, hipStream_t s);
// lds: stage in LDS (the caller has checked rell_lds_fits); returns the HIP error of the launch set-up
hipError_t launch_rell(const RellReq &r, bool lds, hipStream_t s);
// whether the LDS path can hold the table: the device's LDS per workgroup less the room kept for static LDS
bool rell_lds_fits(int N, int tpad, int device);
// isig[u][t] = isig[t][u] = 1 / sigma_ut for u < t < T, sigma_ut^2 = N / (N - 1) * sum_s (d_s - mean)^2 with d_s = X[s][u] - X[s][t]
// and mean = (sum_s d_s) / N: two passes over the centred differences, plain f64, a fixed summation order (k_rell_pairsd: a
// workgroup per 4 x 4 tile of pairs, its threads strided over the sites).  N = 1 or a zero sum of squares (identical columns)
// gives 0; so do the diagonal and the padding column.  The whole [tpad][tpad] matrix is written.
void launch_rell_pairsd(const double *X, double *isig, int N, int T, int tpad, hipStream_t s);
// the weighted arm; lds as for launch_rell, after rell_weighted_lds_fits (table plus matrix)
hipError_t launch_rell_weighted(const RellWReq &r, bool lds, hipStream_t s);
bool rell_weighted_lds_fits(int N, int tpad, int device);

// start / stop (launch_pmat, launch_oplist without ctl, launch_reduce; both or neither): timing events that the kernel's own
// dispatch records its start and end in.  Unlike hipEventRecord before and after the launch this puts no marker packets into
// the queue between two kernels (Ctx::tic_self)
// per_request: the requests carry their own models (PmatReq::md), `model` is ignored
void launch_pmat(const ModelDev *model, const PmatReq *reqs, double *frags, int n, hipStream_t s, bool per_request = false,
                 hipEvent_t start = nullptr, hipEvent_t stop = nullptr);
// n models built from their requests (device memory), one wavefront each; follow it with launch_eigfrags_n
void launch_model_build(const ModelReq *reqs, int n, hipStream_t s, hipEvent_t start = nullptr, hipEvent_t stop = nullptr);
// constant fragment sets for the eigen-basis transforms used by the sumtable:
//   set 0: x_i = sum_s pi_s U[s][i] A[s]     set 1: y_i = sum_j Uinv[i][j] B[j]
void launch_eigfrags(const ModelDev *model, double *frags2, hipStream_t s);
// n models in an array, n x 2*PFRAG doubles out
void launch_eigfrags_n(const ModelDev *models, double *frags2, int n, hipStream_t s);
// any_pitch: some op has an SK_PITCH side (two more LDS fragment regions are allocated)
// ctl != null: the launch has fused Newton tails (OPF_FUSED_NEWTON): chained variant, (gene, tile) claimed by ticket
void launch_oplist(const NvOp *ops, const GeneRun *runs, int nruns, int max_mpad, bool any_pitch, bool chained, hipStream_t s, NewtonCtl *ctl = nullptr,
                   hipEvent_t start = nullptr, hipEvent_t stop = nullptr);
void launch_reduce(const ReduceReq *reqs, int n, hipStream_t s, hipEvent_t start = nullptr, hipEvent_t stop = nullptr);
// tickets: request index per ticket, register-form tickets [0, nreg) then streaming-form [nreg, nreg + nstream)
void launch_newton(const ModelDev *model, const NewtonReq *reqs, const int *tickets, int nreg, int nstream, NewtonCtl *ctl, hipStream_t s);
// the no-exchange fallback: one workgroup per listed request (register-form requests first), same bits as the split form
void launch_newton_seq(const ModelDev *model, const NewtonReq *reqs, const int *req_list, int nreg, int nstream, NewtonCtl *ctl, hipStream_t s);

// The MinHash path (mash.hip; the rule is in include/peprml.h, the shared pieces in mash.hpp).  A batch of genomes is one byte
// buffer, every record followed by MASH_SEP; values[] has one entry per byte.  A span is a run of whole tiles of one genome.
struct MashSpan { unsigned begin, end; int genome; };
void launch_mash_hash(const uint8_t *bytes, unsigned nbytes, const MashSpan *spans, int nspans, int k, uint64_t *values, unsigned long long *nvalid, unsigned *hist,
                      hipStream_t s);
void launch_mash_cut(const unsigned *hist, const unsigned long long *nvalid, const int *min_bins, int ngenomes, int s, int *cut_bins, unsigned *count, hipStream_t st);
void launch_mash_compact(const uint64_t *values, const MashSpan *spans, int nspans, const unsigned *first, const int *cut_bins, int k, uint64_t *comp, unsigned *count,
                         hipStream_t s);
// tmp == nullptr: only tmp_bytes is set.  Sorts comp[first[g] .. first[g] + count[g]) of every genome into sorted[] at the same place
hipError_t launch_mash_sort(void *tmp, size_t &tmp_bytes, const uint64_t *comp, uint64_t *sorted, unsigned total, int ngenomes, const unsigned *first,
                            const unsigned *count, unsigned *seg_end, int k, hipStream_t s);
void launch_mash_unique(const uint64_t *sorted, const unsigned *first, const unsigned *count, int ngenomes, int s, uint64_t *sketch, int *len, hipStream_t st);
// out[r * ncols + c] = (common, denom) of the sketches rows[r] and cols[c]; nrows <= 65535
void launch_mash_pairs(const uint64_t *sketch, const int *len, const int *rows, int nrows, const int *cols, int ncols, int s, int2 *out, hipStream_t st);

// Markov clustering (mcl.hip; the rule is in include/peprml.h, the shared pieces in mcl.hpp).  A sub-batch's components: mat =
// the offset in doubles of its matrix in the pool (column major, column stride npad; LDS classes: npad = n, one matrix; HBM class:
// npad = n rounded up to MCL_TILE, two matrices, the second behind the first), col0 = its first column in the call's per-column
// arrays (the CSR's ptr, best, chaos_col), mask_off = its first word in the call's masks (n x mcl_words(n) words)
struct MclComp { long long mat; int n, npad, col0, pad; long long mask_off; };
struct MclRun { double inflation, prune_inverse, chaos_eps; int max_iter, pad; };
size_t mcl_lds_bytes(bool packed);
void launch_mcl_fill(const MclComp *comps, int ncomps, int max_n, const long long *ptr, const int *row, const double *val, double *pool, hipStream_t s);
// the whole iteration and the reading of ncomps components of a class in one launch; n <= MCL_PACKED_MAX (packed) or MCL_LDS_MAX.
// iters / chaos: per component of the sub-batch.  write_back: the final matrices replace the start matrices in the pool
hipError_t launch_mcl_lds(bool packed, const MclComp *comps, int ncomps, double *pool, const MclRun &run, int *best, unsigned *mask, int *iters, double *chaos,
                          bool write_back, hipStream_t s);
// one iteration of the HBM class over the components active[0 .. nactive): parity 0 reads the first matrix and writes the second
void launch_mcl_expand(const MclComp *comps, const int *active, int nactive, int max_npad, double *pool, int parity, hipStream_t s);
void launch_mcl_inflate(const MclComp *comps, const int *active, int nactive, int max_n, double *pool, int parity, const MclRun &run, double *chaos_col, hipStream_t s);
// iters[component] = it, chaos[component], flag[position in active] = chaos < chaos_eps
void launch_mcl_flag(const MclComp *comps, const int *active, int nactive, const double *chaos_col, const MclRun &run, int it, int *iters, double *chaos, int *flag,
                     hipStream_t s);
void launch_mcl_read(const MclComp *comps, int ncomps, int max_n, const double *pool, const int *iters, int *best, unsigned *mask, hipStream_t s);

// Homology search (sw.hip; the rule is in include/peprml.h, the shared pieces in sw.hpp).  A chunk: `len` stream bytes at `off` of
// the call's stream array (one genome's subjects back to back, SW_MARK behind each), its first subject in the per-subject
// position array, its genome.  A query: its codes in the residue array, its row in best / dbg, and for a query of several
// passes the offset (in int2) of its line buffers, where chunk c's begins at lb_at(c) - run.lb_base (-1: one pass, none)
struct SwChunk { long long off; int len, sub0, genome, lb_at; };
struct SwQuery { long long off; int len, index; long long lb_off; };
struct SwRun { int oe, ext, G, nq, chunk0, pad; long long lb_base, dbg_ld; };
// class cls: queries[0 .. run.nq) against chunks[run.chunk0 .. run.chunk0 + nchunks); best[index * G + genome] takes the
// 64-bit maximum of the chunk's keys; dbg (test door, else null): dbg[index * dbg_ld + position] = the pair's score
void launch_sw_score(int cls, const SwQuery *queries, const SwChunk *chunks, int nchunks, const SwRun &run, const uint8_t *codes, const uint8_t *stream,
                     const int *sub_pos, const int8_t *table, int2 *linebuf, unsigned long long *best, int *dbg, hipStream_t s);

// Multiple alignment (msa.hip; the rule is in include/peprml.h, the shared pieces in msa.hpp).  A cluster's rows are n x L codes
// (row major, MSA_GAP in a gap cell), its counts and a V are 12 dwords a column: 24 int16, code a in half a & 1 of dword a / 2.
// A task is one merge: dir = its npass x (LY + lanes - 1) x lanes direction words, word ((pass * (LY + lanes - 1) + step) * lanes
// + lane), step = column + lane; lb = two line buffers of LY (H, F) pairs (null: one pass); map = LX + LY (column of X, column of
// Y) pairs, -1 for a gap, filled from the end; info[task] = (merged length, score)
struct MsaCluster { const uint8_t *rows; uint32_t *cnt; int n, L; };
struct MsaTask {
    const uint8_t *x_rows, *y_rows; uint8_t *out_rows;
    const uint32_t *x_cnt, *y_cnt; uint32_t *out_cnt;
    uint32_t *v, *dir;
    int2 *lb, *map;
    int LX, LY, nX, nY, GO, GE, cls, pad;
};
struct MsaBlock { int first, count, cls, pad; };      // a workgroup of k_msa_dp: tasks[first .. first + count) of one class, count <= 64 / lanes
void launch_msa_counts(const MsaCluster *clusters, int nclusters, int max_L, hipStream_t s);
void launch_msa_colv(const MsaTask *tasks, int ntasks, int max_LY, const int8_t *table576, hipStream_t s);
void launch_msa_dp(const MsaTask *tasks, const MsaBlock *blocks, int nblocks, int2 *info, hipStream_t s);
void launch_msa_walk(const MsaTask *tasks, int ntasks, int2 *info, hipStream_t s);
void launch_msa_gather(const MsaTask *tasks, int ntasks, int max_L, const int2 *info, hipStream_t s);

}  // namespace pml
