"""ctypes binding of include/mi_phylo.h (the C ABI of libmi_phylo.so).

There is no CPU fallback: if the HIP library is missing the import fails loudly.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# MI_PHYLO_LIBRARY: another build of the same library (kernel A/B runs: tools/ab_kernels.py)
LIB_PATH = os.environ.get("MI_PHYLO_LIBRARY") or os.path.join(_HERE, "libmi_phylo.so")

I32P = C.POINTER(C.c_int32)
F64P = C.POINTER(C.c_double)


class EngineSpec(C.Structure):
    """mi_engine_spec (include/mi_phylo.h)."""
    _fields_ = [(k, C.c_int32) for k in (
        "taxon_count", "pattern_count", "state_count", "category_count", "subst_model",
        "site_model", "clock_model", "use_tip_states", "device", "reserved")]


class BranchOptOptions(C.Structure):
    """mi_branch_opt_options (include/mi_phylo.h)."""
    _fields_ = [("max_iterations", C.c_int32), ("check_interval", C.c_int32),
                ("pack_active", C.c_int32), ("tolerance", C.c_double), ("min_length", C.c_double),
                ("max_length", C.c_double), ("reserved", C.c_int32 * 4)]


class NniSearchOptions(C.Structure):
    """mi_nni_search_options (include/mi_phylo.h)."""
    _fields_ = [("max_moves", C.c_int32), ("pack_active", C.c_int32), ("min_gain", C.c_double),
                ("reserved", C.c_int32 * 4), ("branch_opt", BranchOptOptions)]


class SprSearchOptions(C.Structure):
    """mi_spr_search_options (include/mi_phylo.h)."""
    _fields_ = [("max_moves", C.c_int32), ("pack_active", C.c_int32), ("min_gain", C.c_double),
                ("radius", C.c_int32), ("reserved", C.c_int32 * 3), ("branch_opt", BranchOptOptions)]


class DistanceOptions(C.Structure):
    """mi_distance_options (include/mi_phylo.h)."""
    _fields_ = [("max_iterations", C.c_int32), ("reserved0", C.c_int32), ("tolerance", C.c_double),
                ("min_length", C.c_double), ("max_length", C.c_double), ("reserved", C.c_int32 * 4)]


class ViOptions(C.Structure):
    """mi_vi_options (include/mi_phylo.h)."""
    _fields_ = [("particle_count", C.c_int32), ("rows", C.c_int32), ("estimator", C.c_int32),
                ("anneal_steps", C.c_int32), ("max_steps", C.c_int32), ("reserved0", C.c_int32),
                ("prior_rate", C.c_double), ("step_size", C.c_double * 2), ("sbn_step_size", C.c_double),
                ("step_decay", C.c_double), ("adam_beta0", C.c_double), ("adam_beta1", C.c_double),
                ("adam_epsilon", C.c_double), ("seed", C.c_uint64), ("first_sample", C.c_int64),
                ("reserved", C.c_int32 * 4)]


# Every symbol include/mi_phylo.h declares: (restype, argtypes)
_V = C.c_void_p
SYMBOLS = {
    "mi_abi_version": (C.c_int32, []),
    "mi_last_error": (C.c_char_p, []),
    "mi_device_count": (C.c_int32, []),
    "mi_device_bytes_held": (C.c_int64, []),
    "mi_engine_create_sharded":
        (C.c_int32, [C.POINTER(EngineSpec), C.c_int32, I32P, C.c_int32, _V, _V, _V, _V, _V,
                     C.POINTER(_V)]),
    "mi_engine_shard_count": (C.c_int32, [_V]),
    "mi_engine_shard_device": (C.c_int32, [_V, C.c_int32]),
    "mi_shard_range": (C.c_int32, [C.c_int32, C.c_int32, C.c_int32, I32P, I32P]),
    "mi_engine_gradients_unrooted_reduced":
        (C.c_int32, [_V, C.c_int32, _V, _V, _V, C.c_int32, _V, _V, C.c_int32, _V, _V, _V]),
    "mi_engine_gradients_unrooted_reduced_device":
        (C.c_int32, [_V, _V, C.c_int32, _V, _V, _V, C.c_int32, _V, _V, C.c_int32, _V, _V, _V]),
    "mi_engine_create": (C.c_int32, [C.POINTER(EngineSpec), _V, _V, _V, C.POINTER(_V)]),
    "mi_engine_create_reversible":
        (C.c_int32, [C.POINTER(EngineSpec), _V, _V, _V, _V, _V, C.POINTER(_V)]),
    "mi_wag_model": (C.c_int32, [F64P, F64P]),
    "mi_engine_destroy": (None, [_V]),
    "mi_engine_param_count": (C.c_int32, [_V]),
    "mi_engine_block_count": (C.c_int32, [_V]),
    "mi_engine_block": (C.c_int32, [_V, C.c_int32, C.POINTER(C.c_char_p), I32P, I32P]),
    "mi_engine_log_likelihoods_unrooted": (C.c_int32, [_V, C.c_int32, _V, _V, _V, C.c_int32, _V]),
    "mi_engine_gradients_unrooted":
        (C.c_int32, [_V, C.c_int32, _V, _V, _V, C.c_int32, _V, _V, _V, _V]),
    "mi_engine_log_likelihoods_rooted":
        (C.c_int32, [_V, C.c_int32, _V, _V, _V, _V, _V, _V, C.c_int32, C.c_int32, _V]),
    "mi_engine_gradients_rooted":
        (C.c_int32, [_V, C.c_int32, _V, _V, _V, _V, _V, _V, _V, _V, C.c_int32, _V, _V, _V, _V,
                     _V]),
    "mi_engine_log_likelihoods_unrooted_device":
        (C.c_int32, [_V, _V, C.c_int32, _V, _V, _V, C.c_int32, _V]),
    "mi_engine_gradients_unrooted_device":
        (C.c_int32, [_V, _V, C.c_int32, _V, _V, _V, C.c_int32, _V, _V, _V, _V]),
    "mi_engine_log_likelihoods_rooted_device":
        (C.c_int32, [_V, _V, C.c_int32, _V, _V, _V, _V, _V, _V, C.c_int32, C.c_int32, _V]),
    "mi_engine_gradients_rooted_device":
        (C.c_int32, [_V, _V, C.c_int32, _V, _V, _V, _V, _V, _V, _V, _V, C.c_int32, _V, _V, _V,
                     _V, _V]),
    "mi_engine_branch_hessian_unrooted":
        (C.c_int32, [_V, C.c_int32, _V, _V, _V, C.c_int32, _V, _V, _V, _V]),
    "mi_engine_branch_hessian_unrooted_device":
        (C.c_int32, [_V, _V, C.c_int32, _V, _V, _V, C.c_int32, _V, _V, _V, _V]),
    "mi_engine_nni_scan_unrooted":
        (C.c_int32, [_V, C.c_int32, _V, _V, _V, C.c_int32, _V, _V, _V]),
    "mi_engine_nni_scan_unrooted_device":
        (C.c_int32, [_V, _V, C.c_int32, _V, _V, _V, C.c_int32, _V, _V, _V]),
    "mi_engine_reserve_nni_scan": (C.c_int32, [_V, C.c_int32]),
    "mi_nni_neighbour": (C.c_int32, [C.c_int32, _V, _V, C.c_int32, C.c_int32, _V, _V]),
    "mi_engine_reserve": (C.c_int32, [_V, C.c_int32, C.c_int32]),
    "mi_engine_reserve_reduced": (C.c_int32, [_V, C.c_int32, C.c_int32]),
    "mi_engine_reserve_hessian": (C.c_int32, [_V, C.c_int32]),
    "mi_engine_optimize_branch_lengths_unrooted":
        (C.c_int32, [_V, C.c_int32, _V, _V, _V, C.c_int32, _V, _V, _V, _V, _V, _V, _V]),
    "mi_engine_optimize_branch_lengths_unrooted_device":
        (C.c_int32, [_V, _V, C.c_int32, _V, _V, _V, C.c_int32, _V, _V, _V, _V, _V, _V, _V]),
    "mi_engine_reserve_branch_opt": (C.c_int32, [_V, C.c_int32]),
    "mi_engine_nni_apply_unrooted": (C.c_int32, [_V, C.c_int32, _V, _V, _V, _V, _V]),
    "mi_engine_nni_apply_unrooted_device": (C.c_int32, [_V, _V, C.c_int32, _V, _V, _V, _V, _V]),
    "mi_engine_nni_search_unrooted":
        (C.c_int32, [_V, C.c_int32, _V, _V, _V, C.c_int32, _V, _V, _V, _V, _V, _V, _V, _V, _V, _V]),
    "mi_engine_nni_search_unrooted_device":
        (C.c_int32, [_V, _V, C.c_int32, _V, _V, _V, C.c_int32, _V, _V, _V, _V, _V, _V, _V, _V, _V,
                     _V]),
    "mi_engine_reserve_nni_search": (C.c_int32, [_V, C.c_int32]),
    "mi_engine_pattern_log_likelihoods_unrooted":
        (C.c_int32, [_V, C.c_int32, _V, _V, _V, C.c_int32, _V, _V]),
    "mi_engine_pattern_log_likelihoods_unrooted_device":
        (C.c_int32, [_V, _V, C.c_int32, _V, _V, _V, C.c_int32, _V, _V]),
    "mi_engine_ancestral_states_unrooted":
        (C.c_int32, [_V, C.c_int32, _V, _V, _V, C.c_int32, _V, _V, _V, _V, _V, _V]),
    "mi_engine_ancestral_states_unrooted_device":
        (C.c_int32, [_V, _V, C.c_int32, _V, _V, _V, C.c_int32, _V, _V, _V, _V, _V, _V]),
    "mi_engine_reserve_ancestral": (C.c_int32, [_V, C.c_int32]),
    "mi_engine_placement_unrooted":
        (C.c_int32, [_V, C.c_int32, _V, _V, _V, C.c_int32, C.c_int32, C.c_int32, _V, _V, _V, C.c_int32, _V,
                     _V, _V, _V, _V, _V, _V]),
    "mi_engine_placement_unrooted_device":
        (C.c_int32, [_V, _V, C.c_int32, _V, _V, _V, C.c_int32, C.c_int32, C.c_int32, _V, _V, _V, C.c_int32,
                     _V, _V, _V, _V, _V, _V, _V]),
    "mi_engine_reserve_placement": (C.c_int32, [_V, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "mi_engine_spr_scan_unrooted":
        (C.c_int32, [_V, C.c_int32, _V, _V, _V, C.c_int32, C.c_int32, _V, _V, _V, _V, _V]),
    "mi_engine_spr_scan_unrooted_device":
        (C.c_int32, [_V, _V, C.c_int32, _V, _V, _V, C.c_int32, C.c_int32, _V, _V, _V, _V, _V]),
    "mi_engine_reserve_spr_scan": (C.c_int32, [_V, C.c_int32]),
    "mi_spr_neighbour": (C.c_int32, [C.c_int32, _V, _V, C.c_int32, C.c_int32, C.c_int32, _V, _V]),
    "mi_engine_spr_apply_unrooted": (C.c_int32, [_V, C.c_int32, _V, _V, _V, _V, _V]),
    "mi_engine_spr_apply_unrooted_device": (C.c_int32, [_V, _V, C.c_int32, _V, _V, _V, _V, _V]),
    "mi_engine_spr_search_unrooted":
        (C.c_int32, [_V, C.c_int32, _V, _V, _V, C.c_int32, _V, _V, _V, _V, _V, _V, _V, _V, _V, _V]),
    "mi_engine_spr_search_unrooted_device":
        (C.c_int32, [_V, _V, C.c_int32, _V, _V, _V, C.c_int32, _V, _V, _V, _V, _V, _V, _V, _V, _V,
                     _V]),
    "mi_engine_reserve_spr_search": (C.c_int32, [_V, C.c_int32]),
    "mi_engine_rell": (C.c_int32, [_V, C.c_int32, C.c_int32, C.c_int32, _V, _V, _V, _V, _V, _V]),
    "mi_engine_rell_device":
        (C.c_int32, [_V, _V, C.c_int32, C.c_int32, C.c_int32, _V, _V, _V, _V, _V, _V]),
    "mi_engine_reserve_rell": (C.c_int32, [_V, C.c_int32, C.c_int32, C.c_int32]),
    "mi_engine_rell_bootstrap_unrooted":
        (C.c_int32, [_V, C.c_int32, _V, _V, _V, C.c_int32, C.c_int32, _V, _V, _V, _V, _V, _V, _V]),
    "mi_engine_bootstrap_weights":
        (C.c_int32, [_V, C.c_int32, _V, C.c_int32, C.c_int64, C.c_uint64, C.c_int64, _V]),
    "mi_engine_bootstrap_weights_device":
        (C.c_int32, [_V, _V, C.c_int32, _V, C.c_int32, C.c_int64, C.c_uint64, C.c_int64, _V]),
    "mi_engine_reserve_bootstrap_weights": (C.c_int32, [_V, C.c_int32, C.c_int32]),
    "mi_engine_topology_tests":
        (C.c_int32, [_V, C.c_int32, C.c_int32, _V, _V, C.c_int32, _V, _V, C.c_uint64, C.c_int64, _V, _V, _V, _V, _V]),
    "mi_engine_topology_tests_device":
        (C.c_int32, [_V, _V, C.c_int32, C.c_int32, _V, _V, C.c_int32, _V, _V, C.c_uint64, C.c_int64, _V, _V, _V, _V,
                     _V]),
    "mi_engine_reserve_topology_tests": (C.c_int32, [_V, C.c_int32, C.c_int32, C.c_int32]),
    "mi_engine_topology_tests_unrooted":
        (C.c_int32, [_V, C.c_int32, _V, _V, _V, C.c_int32, C.c_int32, _V, _V, C.c_uint64, C.c_int64, _V, _V, _V, _V,
                     _V, _V, _V]),
    "mi_engine_pattern_mixture": (C.c_int32, [_V, C.c_int32, C.c_int32, _V, _V, _V, _V, _V]),
    "mi_engine_pattern_mixture_device":
        (C.c_int32, [_V, _V, C.c_int32, C.c_int32, _V, _V, _V, _V, _V]),
    "mi_engine_pairwise_distances": (C.c_int32, [_V, C.c_int32, _V, _V, _V, _V, _V, _V]),
    "mi_engine_pairwise_distances_device": (C.c_int32, [_V, _V, C.c_int32, _V, _V, _V, _V, _V, _V]),
    "mi_engine_neighbour_joining":
        (C.c_int32, [_V, C.c_int32, C.c_int32, _V, C.c_double, C.c_double, _V, _V]),
    "mi_engine_neighbour_joining_device":
        (C.c_int32, [_V, _V, C.c_int32, C.c_int32, _V, C.c_double, C.c_double, _V, _V]),
    "mi_engine_starting_trees_unrooted": (C.c_int32, [_V, C.c_int32, _V, _V, _V, _V, _V, _V]),
    "mi_engine_starting_trees_unrooted_device":
        (C.c_int32, [_V, _V, C.c_int32, _V, _V, _V, _V, _V, _V]),
    "mi_engine_reserve_start_trees": (C.c_int32, [_V, C.c_int32]),
    "mi_engine_split_index":
        (C.c_int32, [_V, C.c_int32, C.c_int32, _V, _V, _V, C.c_int32, _V, _V, _V, _V, _V, _V]),
    "mi_engine_split_index_device":
        (C.c_int32, [_V, _V, C.c_int32, C.c_int32, _V, _V, _V, C.c_int32, _V, _V, _V, _V, _V, _V]),
    "mi_engine_rf_distances": (C.c_int32, [_V, C.c_int32, C.c_int32, _V, _V, _V, _V]),
    "mi_engine_rf_distances_device": (C.c_int32, [_V, _V, C.c_int32, C.c_int32, _V, _V, _V, _V]),
    "mi_engine_reserve_splits": (C.c_int32, [_V, C.c_int32, C.c_int32]),
    "mi_engine_sbn_index":
        (C.c_int32, [_V, C.c_int32, C.c_int32, _V, C.c_int32, C.c_int32, C.c_int32, _V, _V, _V, _V, _V, _V, _V]),
    "mi_engine_sbn_index_device":
        (C.c_int32, [_V, _V, C.c_int32, C.c_int32, _V, C.c_int32, C.c_int32, C.c_int32, _V, _V, _V, _V, _V, _V,
                     _V]),
    "mi_engine_sbn_log_prob":
        (C.c_int32, [_V, C.c_int32, C.c_int32, _V, _V, _V, C.c_int32, C.c_int32, C.c_int32, _V, _V, C.c_int32,
                     _V, _V, _V, _V]),
    "mi_engine_sbn_log_prob_device":
        (C.c_int32, [_V, _V, C.c_int32, C.c_int32, _V, _V, _V, C.c_int32, C.c_int32, C.c_int32, _V, _V,
                     C.c_int32, _V, _V, _V, _V]),
    "mi_engine_sbn_normalize": (C.c_int32, [_V, C.c_int32, C.c_int32, C.c_int32, _V, _V, _V]),
    "mi_engine_sbn_normalize_device": (C.c_int32, [_V, _V, C.c_int32, C.c_int32, C.c_int32, _V, _V, _V]),
    "mi_engine_sbn_train":
        (C.c_int32, [_V, C.c_int32, C.c_int32, _V, _V, _V, C.c_int32, C.c_int32, C.c_int32, _V, _V, C.c_int32,
                     C.c_double, C.c_int32, C.c_double, _V, _V, _V]),
    "mi_engine_sbn_train_device":
        (C.c_int32, [_V, _V, C.c_int32, C.c_int32, _V, _V, _V, C.c_int32, C.c_int32, C.c_int32, _V, _V,
                     C.c_int32, C.c_double, C.c_int32, C.c_double, _V, _V, _V]),
    "mi_engine_reserve_sbn": (C.c_int32, [_V, C.c_int32, C.c_int32]),
    "mi_engine_sbn_descent":
        (C.c_int32, [_V, C.c_int32, C.c_int32, _V, _V, _V, C.c_int32, C.c_int32, _V, _V]),
    "mi_engine_sbn_descent_device":
        (C.c_int32, [_V, _V, C.c_int32, C.c_int32, _V, _V, _V, C.c_int32, C.c_int32, _V, _V]),
    "mi_engine_sbn_sample":
        (C.c_int32, [_V, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _V, _V, _V, C.c_uint64, C.c_int64,
                     _V, _V, _V, _V, _V]),
    "mi_engine_sbn_sample_device":
        (C.c_int32, [_V, _V, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _V, _V, _V, C.c_uint64,
                     C.c_int64, _V, _V, _V, _V, _V]),
    "mi_engine_sbn_topology_gradient":
        (C.c_int32, [_V, C.c_int32, C.c_int32, _V, _V, _V, C.c_int32, C.c_int32, C.c_int32, _V, _V, C.c_int32,
                     _V, C.c_int32, _V, _V, _V]),
    "mi_engine_sbn_topology_gradient_device":
        (C.c_int32, [_V, _V, C.c_int32, C.c_int32, _V, _V, _V, C.c_int32, C.c_int32, C.c_int32, _V, _V,
                     C.c_int32, _V, C.c_int32, _V, _V, _V]),
    "mi_engine_psp_table": (C.c_int32, [_V, C.c_int32, C.c_int32, _V, _V, _V]),
    "mi_engine_psp_table_device": (C.c_int32, [_V, _V, C.c_int32, C.c_int32, _V, _V, _V]),
    "mi_engine_psp_index":
        (C.c_int32, [_V, C.c_int32, C.c_int32, _V, _V, C.c_int32, C.c_int32, _V, C.c_int32, C.c_int32, _V]),
    "mi_engine_psp_index_device":
        (C.c_int32, [_V, _V, C.c_int32, C.c_int32, _V, _V, C.c_int32, C.c_int32, _V, C.c_int32, C.c_int32, _V]),
    "mi_engine_branch_model_sample":
        (C.c_int32, [_V, C.c_int32, C.c_int32, C.c_int32, _V, C.c_int32, _V, C.c_uint64, C.c_int64, C.c_double,
                     _V, _V, _V, _V, _V]),
    "mi_engine_branch_model_sample_device":
        (C.c_int32, [_V, _V, C.c_int32, C.c_int32, C.c_int32, _V, C.c_int32, _V, C.c_uint64, C.c_int64, C.c_double,
                     _V, _V, _V, _V, _V]),
    "mi_engine_branch_model_gradient":
        (C.c_int32, [_V, C.c_int32, C.c_int32, C.c_int32, _V, C.c_int32, _V, _V, _V, _V, _V, _V, _V, _V, _V,
                     C.c_double, C.c_double, _V, _V]),
    "mi_engine_branch_model_gradient_device":
        (C.c_int32, [_V, _V, C.c_int32, C.c_int32, C.c_int32, _V, C.c_int32, _V, _V, _V, _V, _V, _V, _V, _V, _V,
                     C.c_double, C.c_double, _V, _V]),
    "mi_engine_reserve_branch_model": (C.c_int32, [_V, C.c_int32, C.c_int32, C.c_int32]),
    "mi_vi_default_options": (C.c_int32, [C.POINTER(ViOptions)]),
    "mi_engine_vi_create":
        (C.c_int32, [_V, C.c_int32, _V, _V, C.c_int32, _V, C.c_int32, _V, C.POINTER(ViOptions), C.POINTER(_V)]),
    "mi_vi_destroy": (None, [_V]),
    "mi_vi_sizes": (C.c_int32, [_V, I32P]),
    "mi_vi_step_device": (C.c_int32, [_V, _V]),
    "mi_vi_fit": (C.c_int32, [_V, C.c_int32, C.c_int32, _V]),
    "mi_vi_trace": (C.c_int32, [_V, C.c_int32, C.c_int32, _V]),
    "mi_vi_update": (C.c_int32, [_V, _V, _V, _V, _V, _V, _V, _V]),
    "mi_vi_update_device": (C.c_int32, [_V, _V, _V, _V, _V, _V, _V, _V, _V]),
    "mi_vi_get_state": (C.c_int32, [_V, _V, _V, _V, _V, _V, _V]),
    "mi_vi_set_state": (C.c_int32, [_V, _V, _V, _V, _V, _V, _V]),
    "mi_vi_particles": (C.c_int32, [_V, _V, _V, _V, _V, _V, _V]),
    "mi_engine_gp_create":
        (C.c_int32, [_V, C.c_int32, C.c_int32, _V, _V, _V, C.c_double, C.POINTER(_V)]),
    "mi_gp_destroy": (None, [_V]),
    "mi_gp_sizes": (C.c_int32, [_V, I32P]),
    "mi_gp_structure": (C.c_int32, [_V, _V, _V, _V, _V, F64P]),
    "mi_gp_strings": (C.c_int32, [_V, C.c_char_p, C.c_int64, C.POINTER(C.c_int64)]),
    "mi_gp_set_branch_lengths": (C.c_int32, [_V, _V, C.c_int32]),
    "mi_gp_get_branch_lengths": (C.c_int32, [_V, _V]),
    "mi_gp_set_sbn_parameters": (C.c_int32, [_V, _V, C.c_int32]),
    "mi_gp_get_sbn_parameters": (C.c_int32, [_V, _V]),
    "mi_gp_node_probabilities": (C.c_int32, [_V, _V, C.c_int32, _V]),
    "mi_gp_inverted_probabilities": (C.c_int32, [_V, _V, C.c_int32, _V]),
    "mi_gp_populate": (C.c_int32, [_V]),
    "mi_gp_populate_device": (C.c_int32, [_V, _V]),
    "mi_gp_likelihoods": (C.c_int32, [_V, _V, _V, _V, _V]),
    "mi_gp_likelihoods_device": (C.c_int32, [_V, _V, _V, _V]),
    "mi_gp_branch_derivatives": (C.c_int32, [_V, _V, _V, _V, _V]),
    "mi_gp_branch_derivatives_device": (C.c_int32, [_V, _V, _V, _V, _V, _V]),
    "mi_gp_estimate_sbn_parameters": (C.c_int32, [_V, _V]),
    "mi_gp_hybrid_requests": (C.c_int32, [_V, _V, _V, I32P]),
    "mi_gp_hybrid_request_count": (C.c_int32, [C.c_int32, C.c_int32, _V, C.c_int64, I32P, C.POINTER(C.c_int64)]),
    "mi_gp_reserve_hybrid": (C.c_int32, [_V]),
    "mi_gp_hybrid_marginals": (C.c_int32, [_V, _V, _V]),
    "mi_gp_hybrid_marginals_device": (C.c_int32, [_V, _V, _V, _V]),
    "mi_gp_estimate_sbn_parameters_hybrid": (C.c_int32, [_V, _V]),
    "mi_gp_optimize_branch_lengths":
        (C.c_int32, [_V, C.POINTER(BranchOptOptions), _V, I32P, I32P]),
    "mi_engine_gp_create_dag": (C.c_int32, [_V, C.c_int32, C.c_int32, _V, _V, C.POINTER(_V)]),
    "mi_gp_reserve_trees": (C.c_int32, [_V, C.c_int32]),
    "mi_gp_topology_count": (C.c_int32, [_V, C.POINTER(C.c_uint64)]),
    "mi_gp_tree_index": (C.c_int32, [_V, C.c_int32, _V, _V, _V]),
    "mi_gp_tree_index_device": (C.c_int32, [_V, _V, C.c_int32, _V, _V, _V]),
    "mi_gp_tree_log_prob": (C.c_int32, [_V, C.c_int32, _V, _V]),
    "mi_gp_tree_log_prob_device": (C.c_int32, [_V, _V, C.c_int32, _V, _V]),
    "mi_gp_tree_branch_lengths": (C.c_int32, [_V, C.c_int32, _V, C.c_double, _V]),
    "mi_gp_tree_branch_lengths_device": (C.c_int32, [_V, _V, C.c_int32, _V, C.c_double, _V]),
    "mi_gp_train_simple_average": (C.c_int32, [_V, C.c_int32, _V, _V, _V]),
    "mi_gp_sample_trees": (C.c_int32, [_V, C.c_int32, C.c_uint64, C.c_int64, _V, _V, _V, _V, _V]),
    "mi_gp_sample_trees_device": (C.c_int32, [_V, _V, C.c_int32, C.c_uint64, C.c_int64, _V, _V, _V, _V, _V]),
    "mi_gp_enumerate_trees": (C.c_int32, [_V, C.c_int64, C.c_int32, _V, _V, _V, _V]),
    "mi_gp_enumerate_trees_device": (C.c_int32, [_V, _V, C.c_int64, C.c_int32, _V, _V, _V, _V]),
    "mi_engine_reserve_deroot": (C.c_int32, [_V, C.c_int32, C.c_int32]),
    "mi_engine_deroot_trees": (C.c_int32, [_V, C.c_int32, C.c_int32, _V, _V, _V, _V, _V]),
    "mi_engine_deroot_trees_device": (C.c_int32, [_V, _V, C.c_int32, C.c_int32, _V, _V, _V, _V, _V]),
    "mi_gp_reserve_vi": (C.c_int32, [_V, C.c_int32]),
    "mi_gp_log_normalize": (C.c_int32, [_V, _V, _V, _V]),
    "mi_gp_log_normalize_device": (C.c_int32, [_V, _V, _V, _V, _V]),
    "mi_gp_branch_sample":
        (C.c_int32, [_V, C.c_int32, _V, _V, C.c_uint64, C.c_int64, C.c_double, _V, _V, _V, _V, _V]),
    "mi_gp_branch_sample_device":
        (C.c_int32, [_V, _V, C.c_int32, _V, _V, C.c_uint64, C.c_int64, C.c_double, _V, _V, _V, _V, _V]),
    "mi_gp_branch_gradient":
        (C.c_int32, [_V, C.c_int32, _V, _V, _V, _V, _V, _V, _V, _V, _V, _V, _V, C.c_double, C.c_double, _V, _V]),
    "mi_gp_branch_gradient_device":
        (C.c_int32, [_V, _V, C.c_int32, _V, _V, _V, _V, _V, _V, _V, _V, _V, _V, _V, C.c_double, C.c_double, _V, _V]),
    "mi_gp_topology_gradient": (C.c_int32, [_V, C.c_int32, _V, _V, _V, C.c_int32, _V, _V]),
    "mi_gp_topology_gradient_device": (C.c_int32, [_V, _V, C.c_int32, _V, _V, _V, C.c_int32, _V, _V]),
    "mi_engine_deroot_trees_mapped": (C.c_int32, [_V, C.c_int32, C.c_int32, _V, _V, _V, _V, _V, _V]),
    "mi_engine_deroot_trees_mapped_device": (C.c_int32, [_V, _V, C.c_int32, C.c_int32, _V, _V, _V, _V, _V, _V]),
    "mi_gp_vi_create":
        (C.c_int32, [_V, _V, C.c_int32, _V, C.c_int32, _V, C.POINTER(ViOptions), C.POINTER(_V)]),
    "mi_gp_vi_particles": (C.c_int32, [_V, _V, _V, _V, _V, _V, _V, _V]),
    "mi_consensus_tree":
        (C.c_int32, [C.c_int32, C.c_int32, _V, _V, C.c_double, C.c_double, I32P, _V, _V]),
    "mi_engine_check_status": (C.c_int32, [_V, _V]),
    "mi_engine_profile_begin": (C.c_int32, [_V, C.c_int32]),
    "mi_engine_profile_collect": (C.c_int32, [_V, F64P, C.c_int32, I32P]),
    "mi_engine_profile_begin_phases": (C.c_int32, [_V, C.c_int32]),
    "mi_engine_profile_collect_phases": (C.c_int32, [_V, F64P, F64P, C.c_int32, I32P, I32P]),
    "mi_engine_last_call_info":
        (C.c_int32, [_V, C.POINTER(C.c_char_p), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "mi_engine_last_call_path": (C.c_char_p, [_V]),
    "mi_engine_last_call_launches": (C.c_int32, [_V, I32P, I32P]),
    "mi_site_pattern_compress":
        (C.c_int32, [C.c_int32, C.c_int32, C.c_int64, _V, I32P, _V, _V, F64P]),
    "mi_site_pattern_compress_device":
        (C.c_int32, [C.c_int32, C.c_int32, C.c_int64, _V, I32P, C.POINTER(_V), C.POINTER(_V), F64P]),
    "mi_device_free": (None, [_V]),
    "mi_engine_create_device_tips": (C.c_int32, [C.POINTER(EngineSpec), _V, _V, C.POINTER(_V)]),
}

_lib = None


def load():
    """Load libmi_phylo.so and bind every declared symbol (raises if absent)."""
    global _lib
    if _lib is not None:
        return _lib
    # One HIP runtime per process: torch ships its own libamdhip64, libmi_phylo.so is linked
    # against /opt/rocm's.  Whichever is loaded FIRST serves both (same SONAME); loaded the
    # other way round, the second runtime finds no device ("No HIP GPUs are available" from
    # torch, or "no HIP device available" from mi_engine_create).  The Python mirror is used
    # next to torch (device tensors, torch.distributed), so when torch is installed it is
    # loaded first; MI_PHYLO_NO_TORCH_PRELOAD=1 skips that for torch-free use.
    import sys
    if "torch" not in sys.modules and os.environ.get("MI_PHYLO_NO_TORCH_PRELOAD") != "1":
        import importlib.util
        if importlib.util.find_spec("torch") is not None:
            import torch  # noqa: F401
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; "
            "g.build()'` (hipcc --offload-arch=gfx950). libsbn_amd has no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def last_error():
    return load().mi_last_error().decode()
