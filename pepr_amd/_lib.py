"""ctypes loader for pepr_amd/libpeprml.so (the C ABI of include/peprml.h).

There is no Python or CPU fallback: if the shared library is missing this raises, and every
likelihood is computed by the HIP kernels inside it.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# PEPRML_LIB: another build of the same library (same-box A/B of kernel variants, tools/bench_ab.sh); never a fallback
SO_PATH = os.environ.get("PEPRML_LIB") or os.path.join(_HERE, "libpeprml.so")

# every symbol include/peprml.h declares (tests check the library exports all of them)
SYMBOLS = [
    "pml_create", "pml_destroy", "pml_strerror", "pml_last_error", "pml_version",
    "pml_score", "pml_optimize", "pml_search",
    "pml_score_batch", "pml_optimize_batch", "pml_search_batch", "pml_result_free",
    "pml_batch_create", "pml_batch_destroy", "pml_batch_size", "pml_batch_npatterns",
    "pml_batch_score", "pml_batch_score_stored", "pml_batch_site_lnl", "pml_batch_set_alpha", "pml_batch_optimize",
    "pml_batch_search", "pml_batch_newick", "pml_batch_root_derivs", "pml_free",
    "pml_rf_distance", "pml_support_tree", "pml_jackknife", "pml_jackknife_draw", "pml_debug_gather", "pml_concatenate", "pml_parsimony", "pml_parsimony_batch", "pml_refine_next", "pml_bootstrap", "pml_coalescing_stats",
    "pml_matrix_parse_paml", "pml_matrix_register", "pml_model_eval", "pml_batch_set_matrix", "pml_batch_get_matrix", "pml_debug_model_build", "pml_newton_fallbacks", "pml_sh_support", "pml_sh_support_batch", "pml_gamma20", "pml_gamma20_batch", "pml_debug_fpenv", "pml_kernel_stats", "pml_kernel_flops", "pml_kernel_stats_reset",
    "pml_au_fit", "pml_rell_tests", "pml_tree_tests", "pml_tree_test_result_free", "pml_debug_rell",
    "pml_rell_tests_weighted", "pml_tree_tests_weighted", "pml_tree_test_weighted_free", "pml_debug_rell_weighted", "pml_catpv_table",
    "pml_jackknife2", "pml_support_tree_rule", "pml_debug_replicate_freqs",
    "pml_search2", "pml_search2_batch", "pml_search_trace_free", "pml_debug_spr_enumerate", "pml_debug_spr_scores",
    "pml_pairscore_table_blosum62", "pml_nj_from_matrix", "pml_pairwise_scores", "pml_nj_tree", "pml_nj_replicates", "pml_nj_jackknife",
    "pml_debug_pairscores", "pml_pairscore_sum_stats",
    "pml_congruence_costs", "pml_congruence_result_free", "pml_congruence_select", "pml_congruence_filter", "pml_debug_column_splits",
    "pml_congruence_ktile",
    "pml_jackknife3", "pml_fitch_stats", "pml_debug_fitch_tips",
    "pml_tree_compare", "pml_tree_compare_one", "pml_tree_compare_result_free", "pml_debug_tree_splits", "pml_tree_splits_free",
    "pml_debug_tree_pair_sums",
    "pml_trim_columns", "pml_trim_result_free", "pml_trim_congruence_filter", "pml_debug_column_flags", "pml_trim_column_flags_host",
    "pml_trim_stats",
    "pml_gblocks_defaults", "pml_gblocks_trim", "pml_debug_gblocks_flags", "pml_gblocks_flags_host", "pml_gblocks_chunk", "pml_gblocks_stats",
    "pml_trim_pipeline",
    "pml_gene_steps", "pml_gene_steps_result_free", "pml_step_thresholds", "pml_step_draws_host", "pml_debug_step_replicates",
    "pml_gene_steps_stats",
    "pml_bootstrap2", "pml_boot_draws_host", "pml_boot_tile", "pml_debug_boot_replicate", "pml_boot_stats",
    "pml_boot_replicate_lnls",
    "pml_mash_tile", "pml_mash_chunk", "pml_mash_sketch", "pml_mash_dist", "pml_mash_distances", "pml_debug_mash_hashes", "pml_debug_mash_full_sort",
    "pml_mash_stats", "pml_mash_murmur3", "pml_mash_hashes_host", "pml_mash_sketch_host", "pml_mash_pair_host", "pml_mash_distance_of",
    "pml_mash_candidate_distances", "pml_mash_expand_ingroup", "pml_mash_pair_stats", "pml_mash_select_outgroup",
    "pml_neighbor_masher", "pml_neighbor_masher_result_free",
    "pml_mcl_cluster", "pml_mcl_cluster_host", "pml_homolog_groups", "pml_homolog_groups_result_free", "pml_hits_filter_host",
    "pml_hits_bidirectional_host", "pml_homolog_select_host", "pml_mcl_class_limits", "pml_debug_mcl_steps", "pml_mcl_stats",
    "pml_sw_search", "pml_sw_search_host", "pml_sw_result_free", "pml_sw_class_limits", "pml_debug_sw_scores", "pml_sw_stats",
    "pml_msa_align", "pml_msa_align_host", "pml_msa_profile_align", "pml_msa_profile_align_host", "pml_msa_guide_tree_host",
    "pml_msa_result_free", "pml_msa_limits", "pml_debug_msa_profile_align", "pml_msa_stats",
]


class MsaOpts(C.Structure):
    _fields_ = [("gap_open", C.c_int), ("gap_extend", C.c_int), ("table576", C.POINTER(C.c_int))]


class MsaSet(C.Structure):
    _fields_ = [("nseq", C.c_int), ("residues", C.POINTER(C.c_char_p))]


class MsaResult(C.Structure):
    _fields_ = [("nrows", C.c_int), ("ncols", C.c_int), ("rows", C.c_void_p), ("nmerges", C.c_int),
                ("merge_x", C.POINTER(C.c_int)), ("merge_y", C.POINTER(C.c_int)), ("merge_level", C.POINTER(C.c_int)),
                ("merge_score", C.POINTER(C.c_longlong)), ("path", C.POINTER(C.c_ubyte))]


class SwOpts(C.Structure):
    _fields_ = [("gap_open", C.c_int), ("gap_extend", C.c_int), ("lambda_", C.c_double), ("K", C.c_double), ("evalue", C.c_double),
                ("hits_per_query", C.c_int), ("traceback", C.c_int), ("table576", C.POINTER(C.c_int))]


class ProteomeSet(C.Structure):
    _fields_ = [("ngenomes", C.c_int), ("genome_off", C.POINTER(C.c_int)), ("labels", C.POINTER(C.c_char_p)), ("residues", C.POINTER(C.c_char_p))]


class SwResult(C.Structure):
    _fields_ = [("nhits", C.c_longlong), ("query", C.POINTER(C.c_int)), ("subject", C.POINTER(C.c_int)), ("target_genome", C.POINTER(C.c_int)),
                ("score", C.POINTER(C.c_int)), ("bits", C.POINTER(C.c_double)), ("evalue", C.POINTER(C.c_double)),
                ("table", C.c_void_p), ("table_bytes", C.c_longlong), ("cells", C.c_longlong)]


class MclOpts(C.Structure):
    _fields_ = [("inflation", C.c_double), ("prune_inverse", C.c_double), ("chaos_eps", C.c_double), ("max_iter", C.c_int), ("pad", C.c_int)]


class HomologGroupsOpts(C.Structure):
    _fields_ = [("table", C.c_char_p), ("table_bytes", C.c_longlong), ("score_field", C.c_int), ("bidirectional", C.c_int), ("mcl", MclOpts),
                ("ntaxon_labels", C.c_int), ("taxon_labels", C.POINTER(C.c_char_p)), ("taxon_of", C.POINTER(C.c_int)),
                ("min_taxa", C.c_int), ("max_taxa", C.c_int), ("rep_only", C.c_int), ("target_ntax", C.c_int), ("target_min_gene", C.c_int)]


class HomologGroupsResult(C.Structure):
    _fields_ = [("nlabels", C.c_int), ("labels", C.POINTER(C.c_char_p)), ("nclusters", C.c_int), ("cluster_off", C.POINTER(C.c_longlong)),
                ("members", C.POINTER(C.c_int)), ("mcl_text", C.c_void_p), ("nkept", C.c_int), ("kept", C.POINTER(C.c_int)),
                ("ncomponents", C.c_int), ("iterations", C.c_int), ("filtered_text", C.c_void_p)]


class Genome(C.Structure):
    _fields_ = [("nrecords", C.c_int), ("records", C.POINTER(C.c_char_p)), ("lengths", C.POINTER(C.c_longlong))]


class NeighborMasherOpts(C.Structure):
    _fields_ = [("n_ingroup", C.c_int), ("n_pool", C.c_int), ("ingroup", C.POINTER(Genome)), ("pool", C.POINTER(Genome)),
                ("ingroup_names", C.POINTER(C.c_char_p)), ("pool_names", C.POINTER(C.c_char_p)),
                ("k", C.c_int), ("s", C.c_int), ("outgroup_count", C.c_int), ("expand_ingroup", C.c_int),
                ("ingroup_only", C.c_int), ("outgroup_only", C.c_int), ("digits", C.c_int)]


class NeighborMasherResult(C.Structure):
    _fields_ = [("n_ingroup", C.c_int), ("ingroup", C.POINTER(C.c_int)), ("n_outgroup", C.c_int), ("outgroup", C.POINTER(C.c_int)),
                ("n_pool", C.c_int), ("candidate_distance", C.POINTER(C.c_double)),
                ("mean", C.c_double), ("sd", C.c_double), ("max", C.c_double),
                ("n_taxa", C.c_int), ("taxa", C.POINTER(C.c_int)),
                ("distance", C.POINTER(C.c_double)), ("common", C.POINTER(C.c_int)), ("denom", C.POINTER(C.c_int)),
                ("sketch_len", C.POINTER(C.c_int)), ("ingroup_tree", C.c_void_p), ("rooted_tree", C.c_void_p)]


class TreeCompareOpts(C.Structure):
    _fields_ = [("window", C.c_int), ("use_lengths", C.c_int), ("want", C.c_int)]


class TreeCompareResult(C.Structure):
    _fields_ = [("nrows", C.c_int), ("ncols", C.c_int), ("ntax", C.c_int),
                ("rf_legacy", C.POINTER(C.c_int)), ("rf_bipartition", C.POINTER(C.c_int)), ("rf_splits", C.POINTER(C.c_int)),
                ("branch_dist", C.POINTER(C.c_double)), ("discrepant_dist", C.POINTER(C.c_double)),
                ("row_blocks", C.c_longlong), ("resident_bytes", C.c_longlong), ("row_bytes", C.c_longlong)]


class TreeSplits(C.Structure):
    _fields_ = [("ntrees", C.c_int), ("ntax", C.c_int), ("words", C.c_int), ("names", C.POINTER(C.c_char_p)),
                ("nrecords", C.c_longlong), ("first", C.POINTER(C.c_longlong)), ("nreal", C.POINTER(C.c_int)),
                ("split_words", C.POINTER(C.c_ulonglong)), ("length", C.POINTER(C.c_double)), ("length_norm", C.POINTER(C.c_double)),
                ("flags", C.POINTER(C.c_int)), ("split_id", C.POINTER(C.c_int))]


class Config(C.Structure):
    _fields_ = [("device", C.c_int), ("profile", C.c_int), ("arena_bytes", C.c_size_t)]


class Alignment(C.Structure):
    _fields_ = [("ntax", C.c_int), ("nsites", C.c_int),
                ("names", C.POINTER(C.c_char_p)), ("rows", C.POINTER(C.c_char_p))]


class Model(C.Structure):
    _fields_ = [("ncat", C.c_int), ("alpha", C.c_double), ("pi_mode", C.c_int)]


class SearchOpts(C.Structure):
    _fields_ = [("optimize_alpha", C.c_int), ("nni", C.c_int), ("spr_radius", C.c_int),
                ("epsilon", C.c_double), ("seed", C.c_uint),
                ("nconstraints", C.c_int), ("constraint_ntax", C.c_int),
                ("constraint_names", C.POINTER(C.c_char_p)), ("constraint_rows", C.POINTER(C.c_char_p))]


class SearchOpts2(C.Structure):
    _fields_ = [("base", SearchOpts), ("radius_mode", C.c_int), ("radius_step", C.c_int), ("radius_max", C.c_int),
                ("thorough", C.c_int), ("thorough_top", C.c_int), ("thorough_radius_max", C.c_int)]


class SearchStep(C.Structure):
    _fields_ = [("phase", C.c_int), ("rmin", C.c_int), ("rmax", C.c_int), ("distance", C.c_int),
                ("lnl_before", C.c_double), ("lnl_after", C.c_double), ("newick_after", C.c_void_p)]


class SearchTrace(C.Structure):
    _fields_ = [("radius_chosen", C.c_int), ("ntrials", C.c_int), ("trial_radius", C.POINTER(C.c_int)),
                ("trial_lnl", C.POINTER(C.c_double)), ("lnl_start", C.c_double), ("nsteps", C.c_int),
                ("steps", C.POINTER(SearchStep))]


class JackknifeOpts(C.Structure):
    _fields_ = [("reps", C.c_int), ("subset_size", C.c_int), ("seed", C.c_ulonglong),
                ("spr_radius_full", C.c_int), ("epsilon", C.c_double),
                ("shard_rank", C.c_int), ("shard_world", C.c_int)]


class JackknifeOpts2(C.Structure):
    _fields_ = [("base", JackknifeOpts), ("support_model", C.POINTER(Model)), ("support_rule", C.c_int)]


class JackknifeOpts3(C.Structure):
    _fields_ = [("base2", JackknifeOpts2), ("full_method", C.c_int), ("support_method", C.c_int), ("parsimony_radius", C.c_int),
                ("pad", C.c_int)]


class BootstrapOpts2(C.Structure):
    _fields_ = [("reps", C.c_int), ("method", C.c_int), ("seed", C.c_ulonglong), ("spr_radius_best", C.c_int),
                ("parsimony_radius", C.c_int), ("epsilon", C.c_double), ("replicate_model", C.POINTER(Model))]


class ParsimonyOpts(C.Structure):
    _fields_ = [("seed", C.c_uint), ("spr_radius", C.c_int)]


class Result(C.Structure):
    _fields_ = [("status", C.c_int), ("lnl", C.c_double), ("alpha", C.c_double),
                ("tree_length", C.c_double), ("npatterns", C.c_int), ("nsites", C.c_int),
                ("newick", C.c_void_p), ("site_lnl", C.POINTER(C.c_double))]


class TreeTestOpts(C.Structure):
    _fields_ = [("nscales", C.c_int), ("scales", C.POINTER(C.c_double)), ("reps_per_scale", C.c_longlong), ("seed", C.c_ulonglong)]


class TreeTestResult(C.Structure):
    _dp, _lp = C.POINTER(C.c_double), C.POINTER(C.c_longlong)
    _fields_ = [("ntrees", C.c_int), ("nscales", C.c_int), ("k1", C.c_int), ("nsites", C.c_longlong), ("reps", C.c_longlong),
                ("scales", _dp), ("ndraws", _lp), ("lnl", _dp), ("obs", _dp),
                ("au", _dp), ("np", _dp), ("bp", _dp), ("kh", _dp), ("sh", _dp), ("pp", _dp),
                ("au_d", _dp), ("au_c", _dp), ("au_rss", _dp), ("au_nused", C.POINTER(C.c_int)), ("rank", C.POINTER(C.c_int)),
                ("bp_count", _lp), ("kh_count", _lp), ("sh_count", _lp)]


class TreeTestWeighted(C.Structure):
    _dp, _lp = C.POINTER(C.c_double), C.POINTER(C.c_longlong)
    _fields_ = [("ntrees", C.c_int), ("wkh", _dp), ("wsh", _dp), ("wkh_count", _lp), ("wsh_count", _lp), ("sigma", _dp),
                ("wkh_other", C.POINTER(C.c_int))]


class CongruenceOpts(C.Structure):
    _fields_ = [("use_hash_mask", C.c_int), ("hash_mask", C.c_ulonglong)]


class CongruenceResult(C.Structure):
    _lp = C.POINTER(C.c_longlong)
    _fields_ = [("ngenes", C.c_int), ("ntax", C.c_int), ("words", C.c_int), ("names", C.POINTER(C.c_char_p)),
                ("cost_sum", _lp), ("mean_cost", _lp), ("nsplits", C.POINTER(C.c_int)), ("cutoff", C.c_int), ("nkept", C.c_longlong),
                ("kept_words", C.POINTER(C.c_ulonglong)), ("kept_count", _lp), ("kept_cost", _lp),
                ("nrecords", C.c_longlong), ("ndistinct", C.c_longlong)]


class TrimResult(C.Structure):
    _ip = C.POINTER(C.c_int)
    _fields_ = [("ngenes", C.c_int), ("ntax", _ip), ("ncols", _ip), ("nkept", _ip), ("kept_cols", C.POINTER(_ip)),
                ("rows", C.POINTER(C.POINTER(C.c_void_p))), ("gap_or_missing", C.POINTER(C.c_longlong))]


class GblocksParams(C.Structure):
    _fields_ = [("b1", C.c_int), ("b2", C.c_int), ("b3", C.c_int), ("b4", C.c_int), ("b0", C.c_int), ("gaps", C.c_int)]


class GeneStepsResult(C.Structure):
    _ip, _lp = C.POINTER(C.c_int), C.POINTER(C.c_longlong)
    _fields_ = [("ngenes", C.c_int), ("ntax", C.c_int), ("names", C.POINTER(C.c_char_p)), ("ncols", C.c_longlong), ("col_start", _lp),
                ("steps", _ip), ("min_steps", _ip), ("gene_steps", _lp), ("gene_beyond", _lp), ("gene_ratio", C.POINTER(C.c_float))]


class StepThresholdOpts(C.Structure):
    _fields_ = [("statistic", C.c_int), ("replace", C.c_int), ("multiple", C.c_int), ("reps", C.c_int), ("alpha", C.c_double),
                ("seed", C.c_ulonglong), ("mask", C.POINTER(C.c_ubyte))]


_lib = None


def load():
    """Returns the loaded library; raises OSError with a clear message when it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO_PATH):
        raise OSError("pepr_amd/libpeprml.so is not built -- run `python -c 'import __graft_entry__ as g; g.build()'` "
                      "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    L = C.CDLL(SO_PATH)
    vp, dp, ip = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int)
    L.pml_create.argtypes = [C.POINTER(Config), C.POINTER(vp)]
    L.pml_destroy.argtypes = [vp]
    L.pml_destroy.restype = None
    L.pml_strerror.restype = C.c_char_p
    L.pml_strerror.argtypes = [C.c_int]
    L.pml_last_error.restype = C.c_char_p
    L.pml_last_error.argtypes = [vp]
    L.pml_version.restype = C.c_char_p
    ap, mp, sp, rp = C.POINTER(Alignment), C.POINTER(Model), C.POINTER(SearchOpts), C.POINTER(Result)
    L.pml_score.argtypes = [vp, ap, C.c_char_p, mp, C.c_int, rp]
    L.pml_optimize.argtypes = [vp, ap, C.c_char_p, mp, sp, rp]
    L.pml_search.argtypes = [vp, ap, C.c_char_p, mp, sp, rp]
    cpp = C.POINTER(C.c_char_p)
    L.pml_score_batch.argtypes = [vp, C.c_int, ap, cpp, mp, C.c_int, rp]
    L.pml_optimize_batch.argtypes = [vp, C.c_int, ap, cpp, mp, sp, rp]
    L.pml_search_batch.argtypes = [vp, C.c_int, ap, cpp, mp, sp, rp]
    L.pml_result_free.argtypes = [rp]
    L.pml_result_free.restype = None
    L.pml_batch_create.argtypes = [vp, C.c_int, ap, cpp, mp, C.POINTER(vp)]
    L.pml_batch_destroy.argtypes = [vp]
    L.pml_batch_destroy.restype = None
    L.pml_batch_size.argtypes = [vp]
    L.pml_batch_npatterns.argtypes = [vp, C.c_int]
    L.pml_batch_score.argtypes = [vp, dp]
    L.pml_batch_score_stored.argtypes = [vp, dp]
    L.pml_batch_site_lnl.argtypes = [vp, C.c_int, dp]
    L.pml_batch_set_alpha.argtypes = [vp, C.c_int, C.c_double]
    L.pml_batch_optimize.argtypes = [vp, sp, dp, dp]
    L.pml_batch_search.argtypes = [vp, sp, dp, dp]
    L.pml_batch_newick.argtypes = [vp, C.c_int, C.c_int, C.POINTER(vp)]
    L.pml_batch_root_derivs.argtypes = [vp, dp, dp, dp]
    L.pml_free.argtypes = [vp]
    L.pml_free.restype = None
    L.pml_rf_distance.argtypes = [C.c_char_p, C.c_char_p, ip]
    L.pml_support_tree.argtypes = [C.c_char_p, C.c_int, cpp, C.c_int, C.POINTER(vp)]
    L.pml_jackknife.argtypes = [vp, C.c_int, ap, mp, C.POINTER(JackknifeOpts), rp, C.POINTER(vp)]
    L.pml_jackknife_draw.argtypes = [C.c_int, C.c_int, C.c_int, C.c_ulonglong, ip]
    L.pml_debug_gather.argtypes = [vp, C.c_int, ap, C.c_int, ip, ip, ip, ip, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    L.pml_jackknife2.argtypes = [vp, C.c_int, ap, mp, C.POINTER(JackknifeOpts2), rp, C.POINTER(vp)]
    L.pml_support_tree_rule.argtypes = [C.c_char_p, C.c_int, cpp, C.c_int, C.c_int, C.POINTER(vp)]
    L.pml_debug_replicate_freqs.argtypes = [vp, C.c_int, ap, C.c_int, ip, C.POINTER(C.c_longlong), dp]
    L.pml_parsimony.argtypes = [vp, ap, C.POINTER(ParsimonyOpts), rp, C.POINTER(C.c_longlong)]
    L.pml_parsimony_batch.argtypes = [vp, C.c_int, ap, C.POINTER(ParsimonyOpts), rp, C.POINTER(C.c_longlong)]
    L.pml_refine_next.argtypes = [C.c_char_p, C.c_int, C.c_int, cpp, C.POINTER(vp), ip, C.POINTER(vp)]
    L.pml_bootstrap.argtypes = [vp, ap, mp, C.c_int, C.c_ulonglong, C.c_int, C.c_double, rp, C.POINTER(vp)]
    L.pml_sh_support.argtypes = [vp, ap, C.c_char_p, mp, C.c_int, C.c_ulonglong, rp]
    L.pml_sh_support_batch.argtypes = [vp, C.c_int, ap, cpp, mp, C.c_int, C.c_ulonglong, rp]
    L.pml_gamma20.argtypes = [vp, ap, C.c_char_p, mp, rp, dp]
    L.pml_gamma20_batch.argtypes = [vp, C.c_int, ap, cpp, mp, rp, dp]
    L.pml_debug_fpenv.argtypes = [C.POINTER(C.c_uint), C.c_int]
    L.pml_concatenate.argtypes = [C.c_int, ap, C.c_int, ip, C.POINTER(vp)]
    L.pml_kernel_stats.argtypes = [vp, C.c_int, C.POINTER(C.c_longlong), dp, dp]
    L.pml_kernel_flops.argtypes = [vp, C.c_int, dp]
    L.pml_kernel_stats_reset.argtypes = [vp]
    L.pml_newton_fallbacks.argtypes = [vp, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
    L.pml_coalescing_stats.argtypes = [vp, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
    L.pml_matrix_parse_paml.argtypes = [C.c_char_p, dp, dp]
    L.pml_matrix_register.argtypes = [vp, C.c_char_p, dp, dp, ip]
    L.pml_model_eval.argtypes = [vp, ap, C.c_char_p, C.c_int, ip, sp, rp, ip]
    L.pml_batch_set_matrix.argtypes = [vp, C.c_int, dp, dp]
    L.pml_batch_get_matrix.argtypes = [vp, C.c_int, dp, dp]
    L.pml_debug_model_build.argtypes = [vp, C.c_int, dp, dp, dp]
    lp, tp, trp = C.POINTER(C.c_longlong), C.POINTER(TreeTestOpts), C.POINTER(TreeTestResult)
    L.pml_au_fit.argtypes = [C.c_int, dp, lp, C.c_longlong, dp, dp, dp, dp, ip]
    L.pml_rell_tests.argtypes = [vp, C.c_longlong, C.c_int, dp, tp, trp]
    L.pml_tree_tests.argtypes = [vp, ap, C.c_int, cpp, mp, sp, tp, trp, dp]
    L.pml_tree_test_result_free.argtypes = [trp]
    L.pml_tree_test_result_free.restype = None
    L.pml_debug_rell.argtypes = [vp, C.c_longlong, C.c_int, dp, C.c_int, lp, C.c_longlong, C.c_ulonglong, C.c_int, dp, lp, lp, lp, ip, dp]
    twp = C.POINTER(TreeTestWeighted)
    L.pml_rell_tests_weighted.argtypes = [vp, C.c_longlong, C.c_int, dp, tp, trp, twp]
    L.pml_tree_tests_weighted.argtypes = [vp, ap, C.c_int, cpp, mp, sp, tp, trp, twp, dp]
    L.pml_tree_test_weighted_free.argtypes = [twp]
    L.pml_tree_test_weighted_free.restype = None
    L.pml_debug_rell_weighted.argtypes = [vp, C.c_longlong, C.c_int, dp, C.c_int, lp, C.c_longlong, C.c_ulonglong, C.c_int, dp, lp, lp, lp, ip, dp,
                                          dp, dp, lp, lp]
    L.pml_catpv_table.argtypes = [trp, twp, C.POINTER(vp)]
    s2p, stp = C.POINTER(SearchOpts2), C.POINTER(SearchTrace)
    L.pml_search2.argtypes = [vp, ap, C.c_char_p, mp, s2p, rp, stp]
    L.pml_search2_batch.argtypes = [vp, C.c_int, ap, cpp, mp, s2p, rp, stp]
    L.pml_search_trace_free.argtypes = [stp]
    L.pml_search_trace_free.restype = None
    L.pml_debug_spr_enumerate.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, cpp, cpp, ip, C.POINTER(vp), C.POINTER(vp)]
    L.pml_debug_spr_scores.argtypes = [vp, ap, C.c_char_p, mp, C.c_char_p, C.c_int, C.c_int, C.c_int, ip, C.POINTER(vp), C.POINTER(vp),
                                       C.POINTER(vp), C.POINTER(vp)]
    L.pml_pairscore_table_blosum62.argtypes = [ip]
    L.pml_nj_from_matrix.argtypes = [C.c_int, cpp, dp, C.c_int, C.c_int, C.POINTER(vp)]
    L.pml_pairwise_scores.argtypes = [vp, ap, ip, dp]
    L.pml_nj_tree.argtypes = [vp, ap, ip, C.c_int, C.POINTER(vp)]
    L.pml_nj_replicates.argtypes = [vp, C.c_int, ap, C.c_int, C.c_int, ip, ip, C.c_int, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    L.pml_nj_jackknife.argtypes = [vp, C.c_int, ap, C.POINTER(JackknifeOpts), ip, C.c_int, C.POINTER(vp), C.POINTER(vp)]
    L.pml_debug_pairscores.argtypes = [vp, ap, ip, C.c_int, lp]
    L.pml_pairscore_sum_stats.argtypes = [vp, lp, dp]
    crp = C.POINTER(CongruenceResult)
    L.pml_congruence_costs.argtypes = [vp, C.c_int, ap, C.POINTER(CongruenceOpts), crp]
    L.pml_congruence_result_free.argtypes = [crp]
    L.pml_congruence_result_free.restype = None
    L.pml_congruence_select.argtypes = [C.c_int, lp, C.c_double, ip, ip, lp]
    L.pml_congruence_filter.argtypes = [vp, C.c_int, ap, C.c_double, ip, crp]
    L.pml_debug_column_splits.argtypes = [vp, ap, C.c_int, cpp, lp, ip, C.POINTER(vp)]
    L.pml_congruence_ktile.argtypes = []
    L.pml_jackknife3.argtypes = [vp, C.c_int, ap, mp, C.POINTER(JackknifeOpts3), rp, C.POINTER(vp), lp]
    L.pml_fitch_stats.argtypes = [vp, lp, lp]
    L.pml_debug_fitch_tips.argtypes = [vp, C.c_int, ap, C.c_int, ip, ip, ip, ip, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    tcp, tco = C.POINTER(TreeCompareResult), C.POINTER(TreeCompareOpts)
    L.pml_tree_compare.argtypes = [vp, C.c_int, cpp, tco, tcp]
    L.pml_tree_compare_one.argtypes = [vp, C.c_char_p, C.c_int, cpp, tco, tcp]
    L.pml_tree_compare_result_free.argtypes = [tcp]
    L.pml_tree_compare_result_free.restype = None
    L.pml_debug_tree_splits.argtypes = [vp, C.c_int, cpp, C.c_int, C.POINTER(TreeSplits)]
    L.pml_tree_splits_free.argtypes = [C.POINTER(TreeSplits)]
    L.pml_tree_splits_free.restype = None
    L.pml_debug_tree_pair_sums.argtypes = [vp, C.c_int, cpp, C.c_int, C.c_int, ip, lp, dp]
    trp2 = C.POINTER(TrimResult)
    L.pml_trim_columns.argtypes = [vp, C.c_int, ap, C.c_int, trp2]
    L.pml_trim_result_free.argtypes = [trp2]
    L.pml_trim_result_free.restype = None
    L.pml_trim_congruence_filter.argtypes = [vp, C.c_int, ap, C.c_int, C.c_double, ip, trp2, crp]
    L.pml_debug_column_flags.argtypes = [vp, ap, C.POINTER(C.c_ubyte)]
    L.pml_trim_column_flags_host.argtypes = [ap, C.POINTER(C.c_ubyte)]
    L.pml_trim_stats.argtypes = [vp, lp, lp, dp]
    gbp, ubp = C.POINTER(GblocksParams), C.POINTER(C.c_ubyte)
    L.pml_gblocks_defaults.argtypes = [C.c_int, gbp]
    L.pml_gblocks_trim.argtypes = [vp, C.c_int, ap, gbp, trp2]
    L.pml_debug_gblocks_flags.argtypes = [vp, ap, gbp, ubp]
    L.pml_gblocks_flags_host.argtypes = [ap, gbp, ubp]
    L.pml_gblocks_chunk.argtypes = []
    L.pml_gblocks_stats.argtypes = [vp, lp, lp, dp]
    L.pml_trim_pipeline.argtypes = [vp, C.c_int, ap, gbp, C.c_int, C.c_int, C.c_double, ip, trp2, trp2, crp]
    gsp, stp = C.POINTER(GeneStepsResult), C.POINTER(StepThresholdOpts)
    L.pml_gene_steps.argtypes = [vp, C.c_int, ap, C.c_char_p, gsp]
    L.pml_gene_steps_result_free.argtypes = [gsp]
    L.pml_gene_steps_result_free.restype = None
    L.pml_step_thresholds.argtypes = [vp, gsp, stp, dp, lp]
    L.pml_step_draws_host.argtypes = [stp, C.c_int, lp, C.c_int, C.c_int, lp]
    L.pml_debug_step_replicates.argtypes = [vp, gsp, stp, C.c_int, dp]
    L.pml_gene_steps_stats.argtypes = [vp, lp, dp]
    L.pml_bootstrap2.argtypes = [vp, C.c_int, ap, mp, C.POINTER(BootstrapOpts2), rp, C.POINTER(vp), lp]
    L.pml_boot_draws_host.argtypes = [C.c_ulonglong, C.c_int, C.c_longlong, C.POINTER(C.c_uint)]
    L.pml_boot_tile.argtypes = []
    L.pml_debug_boot_replicate.argtypes = [vp, C.c_int, ap, C.c_int, ip, C.c_ulonglong, C.c_int, C.c_int, ip, ip, ip] + [C.POINTER(vp)] * 6
    L.pml_boot_stats.argtypes = [vp, lp, dp, dp]
    L.pml_boot_replicate_lnls.argtypes = [vp, C.c_int, dp]
    gp, up, ulp = C.POINTER(Genome), C.POINTER(C.c_ubyte), C.POINTER(C.c_ulonglong)
    L.pml_mash_tile.argtypes = []
    L.pml_mash_chunk.argtypes = []
    L.pml_mash_sketch.argtypes = [vp, C.c_int, gp, C.c_int, C.c_int, ulp, ip]
    L.pml_mash_dist.argtypes = [vp, C.c_int, ulp, ip, C.c_int, ulp, ip, C.c_int, C.c_int, C.c_int, ip, ip, dp]
    L.pml_mash_distances.argtypes = [vp, C.c_int, gp, C.c_int, gp, C.c_int, C.c_int, C.c_int, ip, ip, dp]
    L.pml_debug_mash_hashes.argtypes = [vp, gp, C.c_int, ulp]
    L.pml_debug_mash_full_sort.argtypes = [vp, C.c_int]
    L.pml_mash_stats.argtypes = [vp, lp, dp, lp]
    L.pml_mash_murmur3.argtypes = [C.c_char_p, C.c_longlong, C.c_uint, ulp]
    L.pml_mash_hashes_host.argtypes = [gp, C.c_int, ulp]
    L.pml_mash_sketch_host.argtypes = [gp, C.c_int, C.c_int, ulp, ip]
    L.pml_mash_pair_host.argtypes = [ulp, C.c_int, ulp, C.c_int, C.c_int, ip, ip]
    L.pml_mash_distance_of.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
    L.pml_mash_distance_of.restype = C.c_double
    L.pml_mash_candidate_distances.argtypes = [C.c_int, C.c_int, dp, dp]
    L.pml_mash_expand_ingroup.argtypes = [C.c_int, C.c_int, dp, up, C.c_int, ip, ip]
    L.pml_mash_pair_stats.argtypes = [C.c_int, dp, dp]
    L.pml_mash_select_outgroup.argtypes = [C.c_int, dp, C.c_double, C.c_double, C.c_int, ip, ip]
    L.pml_neighbor_masher.argtypes = [vp, C.POINTER(NeighborMasherOpts), C.POINTER(NeighborMasherResult)]
    L.pml_neighbor_masher_result_free.argtypes = [C.POINTER(NeighborMasherResult)]
    L.pml_neighbor_masher_result_free.restype = None
    mop = C.POINTER(MclOpts)
    L.pml_mcl_cluster.argtypes = [vp, C.c_int, C.c_longlong, ip, ip, dp, mop, ip, ip, ip]
    L.pml_mcl_cluster_host.argtypes = [C.c_int, C.c_longlong, ip, ip, dp, mop, ip, ip, ip]
    L.pml_homolog_groups.argtypes = [vp, C.POINTER(HomologGroupsOpts), C.POINTER(HomologGroupsResult)]
    L.pml_homolog_groups_result_free.argtypes = [C.POINTER(HomologGroupsResult)]
    L.pml_homolog_groups_result_free.restype = None
    L.pml_hits_filter_host.argtypes = [C.c_char_p, C.c_longlong, C.POINTER(vp)]
    L.pml_hits_bidirectional_host.argtypes = [C.c_char_p, C.c_longlong, C.c_int, C.POINTER(vp)]
    L.pml_homolog_select_host.argtypes = [C.c_int, lp, ip, ip, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, ip, ip]
    L.pml_mcl_class_limits.argtypes = [ip]
    L.pml_debug_mcl_steps.argtypes = [vp, C.c_int, dp, mop, C.c_int, C.c_int, dp, dp]
    L.pml_mcl_stats.argtypes = [vp, lp, dp]
    sop, psp, srp = C.POINTER(SwOpts), C.POINTER(ProteomeSet), C.POINTER(SwResult)
    L.pml_sw_search.argtypes = [vp, psp, sop, srp]
    L.pml_sw_search_host.argtypes = [psp, sop, srp]
    L.pml_sw_result_free.argtypes = [srp]
    L.pml_sw_result_free.restype = None
    L.pml_sw_class_limits.argtypes = [ip]
    L.pml_debug_sw_scores.argtypes = [vp, C.c_int, cpp, C.c_int, cpp, sop, C.c_int, C.c_int, ip]
    L.pml_sw_stats.argtypes = [vp, lp, lp, dp]
    mo, ms, mr = C.POINTER(MsaOpts), C.POINTER(MsaSet), C.POINTER(MsaResult)
    L.pml_msa_align.argtypes = [vp, C.c_int, ms, mo, mr]
    L.pml_msa_align_host.argtypes = [C.c_int, ms, mo, mr, C.c_char_p, C.c_int]
    L.pml_msa_profile_align.argtypes = [vp, ms, ms, mo, lp, mr]
    L.pml_msa_profile_align_host.argtypes = [ms, ms, mo, lp, mr, C.c_char_p, C.c_int]
    L.pml_msa_guide_tree_host.argtypes = [C.c_int, lp, ip, ip, ip]
    L.pml_msa_result_free.argtypes = [mr]
    L.pml_msa_result_free.restype = None
    L.pml_msa_limits.argtypes = [ip]
    L.pml_debug_msa_profile_align.argtypes = [vp, ms, ms, mo, C.c_int, lp, mr]
    L.pml_msa_stats.argtypes = [vp, lp, dp]
    _lib = L
    return L
