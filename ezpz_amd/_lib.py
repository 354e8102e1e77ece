"""ctypes binding of include/ezpz_amd.h.  The library is required: there is no Python/CPU fallback."""
import ctypes as C
import os

import numpy as np

from . import build as _build

CONSTRAINT_DTYPE = np.dtype(
    [("kind", "<u2"), ("tag", "u1"), ("flags", "u1"), ("priority", "<u4"), ("ids", "<u4", (8,)), ("param", "<f8"),
     ("weight", "<f8")]
)
assert CONSTRAINT_DTYPE.itemsize == 56
STATUS_DTYPE = np.dtype(
    [("iterations", "<u4"), ("converged", "<u4"), ("n_unsatisfied", "<u4"), ("n_warnings", "<u4"),
     ("final_residual_inf", "<f8"), ("final_lambda", "<f8")]
)
assert STATUS_DTYPE.itemsize == 32
GUARD_STEP_DTYPE = np.dtype([("reached", "<f8"), ("attempts", "<u4"), ("accepted", "<u4")])  # EzpzGuardStep
assert GUARD_STEP_DTYPE.itemsize == 16
MC_DIST_DTYPE = np.dtype([("kind", "<u4"), ("reserved", "<u4"), ("a", "<f8"), ("b", "<f8")])  # EzpzMcDist
MC_STATS_DTYPE = np.dtype([("n_valid", "<u8"), ("n_in", "<u8"), ("argmin", "<u8"), ("argmax", "<u8"), ("nominal", "<f8"),
                           ("sum_d", "<f8"), ("sum_d2", "<f8"), ("mean", "<f8"), ("var", "<f8"), ("min", "<f8"), ("max", "<f8")])  # EzpzMcStats
MC_TOTALS_DTYPE = np.dtype([("samples", "<u8"), ("n_ok", "<u8"), ("n_all_in", "<u8")])  # EzpzMcTotals
assert MC_DIST_DTYPE.itemsize == 24 and MC_STATS_DTYPE.itemsize == 88 and MC_TOTALS_DTYPE.itemsize == 24
MC_MOMENTS_INFO_DTYPE = np.dtype([("samples", "<u8"), ("n_complete", "<u8")])  # EzpzMcMomentsInfo
MC_MOMENT_MAX = 64  # EZPZ_MC_MOMENT_MAX
MC_SEQUENCE = 1  # EZPZ_MC_SEQUENCE: bit 0 of EzpzMcDist.reserved
assert MC_MOMENTS_INFO_DTYPE.itemsize == 16
BRANCH_INFO_DTYPE = np.dtype([("samples", "<u8"), ("n_ok", "<u8"), ("n_branches", "<u8"), ("n_overflow", "<u8")])  # EzpzBranchInfo
BRANCH_DTYPE = np.dtype([("first", "<u8"), ("count", "<u8"), ("dist_inf", "<f8"), ("status", STATUS_DTYPE)])  # EzpzBranch
assert BRANCH_INFO_DTYPE.itemsize == 32 and BRANCH_DTYPE.itemsize == 56
BRANCH_MAX, BRANCH_NOT_OK, BRANCH_OVERFLOW = 256, -1, -2  # EZPZ_BRANCH_*


class CConfig(C.Structure):
    _fields_ = [("max_iterations", C.c_uint64), ("residual_tolerance", C.c_double), ("step_tolerance", C.c_double),
                ("initial_lambda", C.c_double)]


class CWarning(C.Structure):
    _fields_ = [("about_constraint", C.c_int32), ("content", C.c_int32)]


class COutcome(C.Structure):
    _fields_ = [("error", C.c_int32), ("err_constraint_id", C.c_int32), ("err_variable", C.c_int64),
                ("iterations", C.c_uint64), ("converged", C.c_int32), ("priority_solved", C.c_uint32),
                ("n_unsatisfied", C.c_uint64), ("n_warnings", C.c_uint64), ("num_vars", C.c_uint64),
                ("num_eqs", C.c_uint64), ("final_lambda", C.c_double), ("final_residual_inf", C.c_double)]


class CSystemInfo(C.Structure):
    _fields_ = [("n_constraints", C.c_uint64), ("n_vars", C.c_uint64), ("n_rows", C.c_uint64), ("nnz_j", C.c_uint64),
                ("nnz_a", C.c_uint64), ("nnz_l", C.c_uint64), ("n_levels", C.c_uint64), ("n_components", C.c_uint64),
                ("program_bytes", C.c_uint64), ("workspace_bytes", C.c_uint64), ("team_size", C.c_uint32),
                ("workspace_in_lds", C.c_uint32), ("team_mode", C.c_uint32), ("n_partitions", C.c_uint32),
                ("program_in_lds", C.c_uint32), ("grid_workgroups", C.c_uint32), ("front_workgroups", C.c_uint32),
                ("front_max_batch", C.c_uint32)]


class CLaunchPolicy(C.Structure):
    _fields_ = [("compute_units", C.c_uint32), ("lanes_min_systems_small", C.c_uint64), ("lanes_min_systems_large", C.c_uint64),
                ("lanes_large_from_vars", C.c_uint32), ("jit_lane_min_batch", C.c_uint64), ("jit_comp_min_batch", C.c_uint64),
                ("jit_comp_min_values", C.c_uint64), ("jit_after_launches", C.c_uint32), ("lane_max_vars", C.c_uint32),
                ("lane_max_constraints", C.c_uint32), ("comp_min_components", C.c_uint32), ("comp_max_component_vars", C.c_uint32),
                ("comp_max_component_constraints", C.c_uint32), ("comp_max_classes", C.c_uint32), ("rec_min_vars_one_solve", C.c_uint32),
                ("rec_min_vars_batch", C.c_uint32), ("rec_one_wavefront_max_vars", C.c_uint32), ("rec_max_components", C.c_uint32),
                ("rec_wide_one_solve_max_vars", C.c_uint32), ("sub_team_max_width", C.c_uint32), ("dense8_max_vars", C.c_uint32),
                ("zero_copy_max_bytes", C.c_uint64), ("h2h_piece_min_bytes", C.c_uint64), ("h2h_piece_max_bytes", C.c_uint64),
                ("h2h_pieces_per_call", C.c_uint32), ("one_call_host_mask_max_constraints", C.c_uint32),
                ("one_call_host_log_max_entries", C.c_uint32), ("front_min_vars_one_solve", C.c_uint32),
                ("front_min_vars_batch", C.c_uint32), ("front_vars_per_workgroup", C.c_uint32), ("front_max_workgroups", C.c_uint32),
                ("front_small_call_wgs_per_round", C.c_uint32)]


class CSensitivityPlan(C.Structure):
    _fields_ = [("n_components", C.c_uint32), ("n_active", C.c_uint32), ("n_small", C.c_uint32), ("n_lds", C.c_uint32),
                ("n_workspace", C.c_uint32), ("max_component_vars", C.c_uint32), ("max_envelope", C.c_uint32),
                ("lds_bytes", C.c_uint32), ("workspace_bytes", C.c_uint64),
                ("route", C.c_uint32), ("front_workgroups", C.c_uint32), ("rhs_per_item", C.c_uint32),
                ("items_per_system", C.c_uint32), ("front_lds_bytes", C.c_uint32)]


class CSweepPlan(C.Structure):
    _fields_ = [("route", C.c_uint32), ("in_kernel", C.c_uint32), ("params_in_lds", C.c_uint32), ("lds_bytes", C.c_uint32)]


class CGuardConfig(C.Structure):
    _fields_ = [("max_halvings", C.c_uint32), ("max_attempts", C.c_uint32), ("max_move", C.c_double)]


class CMcConfig(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("chunk", C.c_uint32), ("hist_bins", C.c_uint32)]


class CMcContribConfig(C.Structure):
    _fields_ = [("pivot_rel", C.c_double), ("reserved", C.c_uint64)]


class CSobolConfig(C.Structure):
    _fields_ = [("seed_b", C.c_uint64), ("reserved", C.c_uint64)]


SOBOL_MAX = 32  # EZPZ_SOBOL_MAX
SOBOL_SEED_B = 0x9E3779B97F4A7C15  # ezpz_default_sobol_config's seed_b; the Python default is seed ^ this


class CMcQuantileConfig(C.Structure):
    _fields_ = [("z", C.c_double), ("reserved", C.c_uint64)]


MC_QUANTILE_MAX_PROBS, MC_QUANTILE_MAX_MEAS = 16, 64  # EZPZ_MC_QUANTILE_MAX_*
MC_QUANTILE_DTYPE = np.dtype([("n_valid", "<u8"), ("rank", "<u8"), ("rank_lo", "<u8"), ("rank_hi", "<u8"), ("frac", "<f8"), ("lo", "<f8"),
                              ("hi", "<f8"), ("value", "<f8"), ("band_lo", "<f8"), ("band_hi", "<f8")])  # EzpzMcQuantile
assert C.sizeof(CMcQuantileConfig) == 16 and MC_QUANTILE_DTYPE.itemsize == 80


class CMcEffectConfig(C.Structure):
    _fields_ = [("bins", C.c_uint32), ("reserved", C.c_uint32)]


MC_EFFECT_MAX_DIM, MC_EFFECT_MAX_BINS, MC_EFFECT_MAX_CELLS = 32, 64, 4096  # the section's limits; EZPZ_MC_EFFECT_MAX_*
assert C.sizeof(CMcEffectConfig) == 8

MC_FACTORIAL_MAX_CORNERS, MC_FACTORIAL_MAX_MEAS = 20, 32  # EZPZ_MC_FACTORIAL_MAX_*
MC_FACTORIAL_DTYPE = np.dtype([("n_valid", "<u8"), ("complete", "<u4"), ("corner_hi", "<u4"), ("corner_lo", "<u4"), ("reserved", "<u4"),
                               ("mean_dev", "<f8"), ("var", "<f8"), ("m_hi", "<f8"), ("m_lo", "<f8")])  # EzpzMcFactorial
assert MC_FACTORIAL_DTYPE.itemsize == 56


class CBranchConfig(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("chunk", C.c_uint32), ("max_branches", C.c_uint32), ("eps_abs", C.c_double), ("eps_rel", C.c_double)]


class CSeekConfig(C.Structure):  # EzpzSeekConfig; the arrays are host pointers, NULL = the default for every entry
    _fields_ = [("weight", C.c_void_p), ("tol", C.c_void_p), ("lo", C.c_void_p), ("hi", C.c_void_p), ("scale", C.c_void_p),
                ("max_iterations", C.c_uint32), ("chunk", C.c_uint32), ("mu0", C.c_double), ("mu_up", C.c_double),
                ("mu_down", C.c_double), ("mu_min", C.c_double), ("mu_max", C.c_double), ("step_tol", C.c_double),
                ("sens_lambda", C.c_double), ("inner", CConfig)]


SEEK_INFO_DTYPE = np.dtype([("status", "<u4"), ("iterations", "<u4"), ("accepted", "<u4"), ("rejected", "<u4"), ("cost0", "<f8"),
                            ("cost", "<f8"), ("worst", "<f8"), ("mu", "<f8")])  # EzpzSeekInfo
assert C.sizeof(CSeekConfig) == 136 and SEEK_INFO_DTYPE.itemsize == 48
SEEK_STATUS = ("REACHED", "MINIMUM", "ITERATIONS", "STALLED", "START_FAILED")  # EZPZ_SEEK_*
SEEK_STEP = ("TRIAL", "MINIMUM", "PIVOT")  # EZPZ_SEEK_STEP_*


class CGuardStep(C.Structure):
    _fields_ = [("reached", C.c_double), ("attempts", C.c_uint32), ("accepted", C.c_uint32)]


SWEEP_ROUTES = ("interpreter", "sub-wavefront teams", "partitioned workgroup", "barrier workgroup", "record walk")  # EZPZ_SWEEP_*
SWEEP_FRONTS = len(SWEEP_ROUTES)  # EZPZ_SWEEP_FRONTS: the route a caller opts into (ezpz_system_set_params_route), behind the entry's own
SWEEP_ROUTE_NAMES = SWEEP_ROUTES + ("fronts",)
PARAMS_ROUTE_DEFAULT, PARAMS_ROUTE_FRONTS = 0, 1  # EZPZ_PARAMS_ROUTE_*
PARAMS_ROUTES = {"default": PARAMS_ROUTE_DEFAULT, "fronts": PARAMS_ROUTE_FRONTS}
SENSITIVITY_ROUTE_DEFAULT, SENSITIVITY_ROUTE_FRONTS = 0, 1  # EZPZ_SENSITIVITY_ROUTE_*
SENSITIVITY_ROUTES = {"default": SENSITIVITY_ROUTE_DEFAULT, "fronts": SENSITIVITY_ROUTE_FRONTS}


class CViewport(C.Structure):
    _fields_ = [("x_min", C.c_double), ("x_max", C.c_double), ("y_min", C.c_double), ("y_max", C.c_double),
                ("width", C.c_uint32), ("height", C.c_uint32)]


class CImageView(C.Structure):  # EzpzImageView
    _fields_ = [("x_min", C.c_double), ("y_min", C.c_double), ("scale", C.c_double), ("width", C.c_uint32), ("height", C.c_uint32)]


DRAW_POINT, DRAW_SEGMENT, DRAW_CIRCLE, DRAW_ARC = 0, 1, 2, 3  # EZPZ_DRAW_*
DRAW_FILL = 1
IMAGE_MAX_LAYERS, IMAGE_MAX_SIDE = 8, 16384  # EZPZ_IMAGE_MAX_*
DRAW_ITEM_DTYPE = np.dtype([("kind", "<u2"), ("layer", "u1"), ("flags", "u1"), ("ids", "<u4", (6,)), ("reserved", "<u4"),
                            ("half_width", "<f8")])  # EzpzDrawItem
IMAGE_INFO_DTYPE = np.dtype([("variants", "<u8"), ("masked", "<u8"), ("items_skipped", "<u8"), ("increments", "<u8")])  # EzpzImageInfo
COMPOSE_LAYER_DTYPE = np.dtype({"names": ["rgb", "opacity", "a_min", "full_at"], "formats": [("u1", (3,)), "u1", "u1", "<u4"],
                                "offsets": [0, 3, 4, 8], "itemsize": 12})  # EzpzComposeLayer
assert C.sizeof(CImageView) == 32 and DRAW_ITEM_DTYPE.itemsize == 40 and IMAGE_INFO_DTYPE.itemsize == 32


class CRedundancyConfig(C.Structure):
    _fields_ = [("rank_tol", C.c_double), ("conflict_tol", C.c_double), ("group_tol", C.c_double)]


# every symbol include/ezpz_amd.h declares
EXPORTS = [
    "ezpz_default_config", "ezpz_device_count", "ezpz_error_string", "ezpz_system_create", "ezpz_system_destroy",
    "ezpz_system_info", "ezpz_system_solve_batch_device", "ezpz_system_solve_batch", "ezpz_solve_inner", "ezpz_solve",
    "ezpz_problem_parse", "ezpz_problem_destroy", "ezpz_problem_num_constraints", "ezpz_problem_num_vars",
    "ezpz_problem_constraints", "ezpz_problem_guesses", "ezpz_problem_num_labels", "ezpz_problem_label",
    "ezpz_analyze", "ezpz_system_eval_batch", "ezpz_system_jacobian_pattern", "ezpz_cache_clear",
    "ezpz_solve_batch",
    "ezpz_current_device",
    "ezpz_solve_analysis",
    "ezpz_system_freedom_batch",
    "ezpz_system_freedom_batch_device",
    "ezpz_resolve_sides",
    "ezpz_system_specialize",
    "ezpz_host_register",
    "ezpz_host_unregister",
    "ezpz_specialized_source",
    "ezpz_multi_create", "ezpz_multi_destroy", "ezpz_multi_device_count", "ezpz_multi_device", "ezpz_multi_shard",
    "ezpz_multi_specialize", "ezpz_multi_solve_batch", "ezpz_system_solve_batch_multi",
    "ezpz_debug_call_trace", "ezpz_launch_policy", "ezpz_debug_front_plan", "ezpz_debug_set_stamps", "ezpz_debug_jit_compilations", "ezpz_debug_freedom_exits",
    "ezpz_mixed_create", "ezpz_mixed_destroy", "ezpz_mixed_total_values", "ezpz_mixed_offsets", "ezpz_mixed_solve_device",
    "ezpz_mixed_solve", "ezpz_system_solve_batch_mixed", "ezpz_multi_solve_batch_mixed",
    "ezpz_system_residual_field", "ezpz_system_residual_field_device", "ezpz_residual_colormap", "ezpz_residual_overlay",
    "ezpz_constraint_has_param", "ezpz_system_solve_batch_params_device", "ezpz_system_solve_batch_params",
    "ezpz_constraint_param_derivative", "ezpz_system_param_sensitivity_plan", "ezpz_system_param_sensitivity_device",
    "ezpz_system_param_sensitivity",
    "ezpz_system_sweep_params_plan", "ezpz_system_sweep_params_device", "ezpz_system_sweep_params",
    "ezpz_default_guard_config", "ezpz_system_sweep_guarded_plan", "ezpz_system_sweep_guarded_device", "ezpz_system_sweep_guarded",
    "ezpz_system_set_params_route",
    "ezpz_system_set_sensitivity_route", "ezpz_debug_front_sens_tables",
    "ezpz_default_redundancy_config", "ezpz_system_redundancy", "ezpz_system_redundancy_device",
    "ezpz_constraint_measure", "ezpz_system_measure", "ezpz_system_measure_device", "ezpz_system_measure_response",
    "ezpz_system_measure_response_device", "ezpz_system_measure_vjp", "ezpz_system_measure_vjp_device",
    "ezpz_default_mc_config", "ezpz_mc_sample", "ezpz_system_tolerance_mc", "ezpz_system_tolerance_mc_device",
    "ezpz_default_mc_contrib_config", "ezpz_mc_contributors", "ezpz_mc_moments", "ezpz_mc_moments_device",
    "ezpz_system_tolerance_mc_contrib", "ezpz_system_tolerance_mc_contrib_device",
    "ezpz_default_sobol_config", "ezpz_mc_sobol_indices", "ezpz_mc_sobol_sums", "ezpz_mc_sobol_sums_device",
    "ezpz_system_tolerance_sobol", "ezpz_system_tolerance_sobol_device",
    "ezpz_default_mc_quantile_config", "ezpz_mc_quantiles", "ezpz_mc_quantiles_device", "ezpz_system_tolerance_mc_quantiles",
    "ezpz_system_tolerance_mc_quantiles_device",
    "ezpz_default_mc_effect_config", "ezpz_mc_effect_indices", "ezpz_mc_effects", "ezpz_mc_effects_device",
    "ezpz_system_tolerance_mc_effects", "ezpz_system_tolerance_mc_effects_device",
    "ezpz_mc_factorial", "ezpz_mc_factorial_device", "ezpz_system_tolerance_mc_factorial", "ezpz_system_tolerance_mc_factorial_device",
    "ezpz_default_seek_config", "ezpz_seek_step", "ezpz_system_seek_targets", "ezpz_system_seek_targets_device",
    "ezpz_default_branch_config", "ezpz_branch_cluster", "ezpz_branch_cluster_device", "ezpz_system_solve_branches",
    "ezpz_system_solve_branches_device",
    "ezpz_sketch_image", "ezpz_sketch_image_device", "ezpz_sketch_image_host", "ezpz_sketch_compose",
    "ezpz_system_tolerance_mc_image", "ezpz_system_tolerance_mc_image_device",
    "ezpz_problem_num_lines", "ezpz_problem_line",
]

_lib = None


def lib():
    """Loads (building first if the sources are newer) libezpz_amd.so.  Raises if it cannot be built/loaded."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("EZPZ_AMD_LIB") or _build.LIB  # EZPZ_AMD_LIB: A/B-test another build of the library
    if path == _build.LIB and os.environ.get("EZPZ_AMD_NO_BUILD") != "1":
        path = _build.build()
    if not os.path.exists(path):
        raise ImportError(f"{path} is missing: run `python -m ezpz_amd.build` (needs hipcc)")
    L = C.CDLL(path)
    vp, sz, u32 = C.c_void_p, C.c_size_t, C.c_uint32
    L.ezpz_default_config.restype = None
    L.ezpz_default_config.argtypes = [C.POINTER(CConfig)]
    L.ezpz_device_count.restype = C.c_int
    L.ezpz_error_string.restype = C.c_char_p
    L.ezpz_error_string.argtypes = [C.c_int]
    L.ezpz_system_create.restype = C.c_int
    L.ezpz_system_create.argtypes = [vp, sz, sz, C.c_int, u32, C.POINTER(vp), C.POINTER(C.c_int32),
                                     C.POINTER(C.c_int64)]
    L.ezpz_system_destroy.restype = None
    L.ezpz_system_destroy.argtypes = [vp]
    L.ezpz_system_info.restype = C.c_int
    L.ezpz_system_info.argtypes = [vp, C.POINTER(CSystemInfo)]
    L.ezpz_solve_batch.restype = C.c_int
    L.ezpz_solve_batch.argtypes = [vp, sz, sz, vp, sz, C.POINTER(CConfig), vp, vp, vp, vp, C.POINTER(C.c_int32),
                                   C.POINTER(C.c_int64)]
    L.ezpz_system_freedom_batch.restype = C.c_int
    L.ezpz_system_freedom_batch.argtypes = [vp, vp, sz, vp, vp]
    L.ezpz_system_freedom_batch_device.restype = C.c_int
    L.ezpz_system_freedom_batch_device.argtypes = [vp, vp, sz, vp, vp, vp, vp]
    L.ezpz_default_redundancy_config.restype = None
    L.ezpz_default_redundancy_config.argtypes = [C.POINTER(CRedundancyConfig)]
    L.ezpz_system_redundancy.restype = C.c_int
    L.ezpz_system_redundancy.argtypes = [vp, vp, sz, C.POINTER(CRedundancyConfig), vp, vp, vp, vp, sz, vp]
    L.ezpz_system_redundancy_device.restype = C.c_int
    L.ezpz_system_redundancy_device.argtypes = [vp, vp, sz, C.POINTER(CRedundancyConfig), vp, vp, vp, vp, sz, vp, vp]
    L.ezpz_constraint_measure.restype = C.c_int
    L.ezpz_constraint_measure.argtypes = [vp, vp, vp, vp, C.POINTER(C.c_int)]
    L.ezpz_system_measure.restype = C.c_int
    L.ezpz_system_measure.argtypes = [vp, vp, sz, vp, sz, vp, vp, vp]
    L.ezpz_system_measure_device.restype = C.c_int
    L.ezpz_system_measure_device.argtypes = [vp, vp, sz, vp, sz, vp, vp, vp, vp]
    L.ezpz_system_measure_response.restype = C.c_int
    L.ezpz_system_measure_response.argtypes = [vp, vp, sz, vp, vp, sz, sz, vp, vp, vp, vp]
    L.ezpz_system_measure_response_device.restype = C.c_int
    L.ezpz_system_measure_response_device.argtypes = [vp, vp, sz, vp, vp, sz, sz, vp, vp, vp, vp, vp]
    L.ezpz_system_measure_vjp.restype = C.c_int
    L.ezpz_system_measure_vjp.argtypes = [vp, vp, sz, vp, vp, sz, vp]
    L.ezpz_system_measure_vjp_device.restype = C.c_int
    L.ezpz_system_measure_vjp_device.argtypes = [vp, vp, sz, vp, vp, sz, vp, vp]
    L.ezpz_default_mc_config.restype = None
    L.ezpz_default_mc_config.argtypes = [C.POINTER(CMcConfig)]
    L.ezpz_mc_sample.restype = C.c_int
    L.ezpz_mc_sample.argtypes = [C.c_uint64, vp, vp, sz, C.c_uint64, sz, vp]
    L.ezpz_system_tolerance_mc.restype = C.c_int
    L.ezpz_system_tolerance_mc.argtypes = [vp, vp, vp, sz, vp, vp, vp, sz, vp, vp, vp, vp, C.c_uint64, C.POINTER(CMcConfig),
                                           C.POINTER(CConfig), vp, vp, vp, vp, vp, vp, vp]
    L.ezpz_system_tolerance_mc_device.restype = C.c_int
    L.ezpz_system_tolerance_mc_device.argtypes = L.ezpz_system_tolerance_mc.argtypes + [vp]
    L.ezpz_default_mc_contrib_config.restype = None
    L.ezpz_default_mc_contrib_config.argtypes = [C.POINTER(CMcContribConfig)]
    L.ezpz_mc_contributors.restype = C.c_int
    L.ezpz_mc_contributors.argtypes = [vp, C.c_uint64, sz, sz, C.POINTER(CMcContribConfig), vp, vp, vp, vp, vp]
    L.ezpz_mc_moments.restype = C.c_int
    L.ezpz_mc_moments.argtypes = [vp, vp, vp, vp, vp, vp, C.c_uint64, sz, sz, u32, vp, vp]
    L.ezpz_mc_moments_device.restype = C.c_int
    L.ezpz_mc_moments_device.argtypes = L.ezpz_mc_moments.argtypes + [vp]
    L.ezpz_system_tolerance_mc_contrib.restype = C.c_int
    L.ezpz_system_tolerance_mc_contrib.argtypes = L.ezpz_system_tolerance_mc.argtypes + [C.POINTER(CMcContribConfig), vp, vp, vp, vp, vp, vp, vp]
    L.ezpz_system_tolerance_mc_contrib_device.restype = C.c_int
    L.ezpz_system_tolerance_mc_contrib_device.argtypes = L.ezpz_system_tolerance_mc_contrib.argtypes + [vp]
    L.ezpz_default_sobol_config.restype = None
    L.ezpz_default_sobol_config.argtypes = [C.POINTER(CSobolConfig)]
    L.ezpz_mc_sobol_indices.restype = C.c_int
    L.ezpz_mc_sobol_indices.argtypes = [vp, vp, sz, sz, vp, vp, vp, vp, vp]
    L.ezpz_mc_sobol_sums.restype = C.c_int
    L.ezpz_mc_sobol_sums.argtypes = [vp, vp, vp, vp, u32, C.c_uint64, sz, sz, u32, vp, vp]
    L.ezpz_mc_sobol_sums_device.restype = C.c_int
    L.ezpz_mc_sobol_sums_device.argtypes = L.ezpz_mc_sobol_sums.argtypes + [vp]
    L.ezpz_system_tolerance_sobol.restype = C.c_int
    L.ezpz_system_tolerance_sobol.argtypes = [vp, vp, vp, sz, vp, vp, vp, sz, C.c_uint64, C.POINTER(CMcConfig), C.POINTER(CConfig),
                                              C.POINTER(CSobolConfig)] + [vp] * 12
    L.ezpz_system_tolerance_sobol_device.restype = C.c_int
    L.ezpz_system_tolerance_sobol_device.argtypes = L.ezpz_system_tolerance_sobol.argtypes + [vp]
    L.ezpz_default_mc_quantile_config.restype = None
    L.ezpz_default_mc_quantile_config.argtypes = [C.POINTER(CMcQuantileConfig)]
    L.ezpz_mc_quantiles.restype = C.c_int
    L.ezpz_mc_quantiles.argtypes = [vp, vp, vp, C.c_uint64, sz, vp, sz, C.POINTER(CMcQuantileConfig), vp]
    L.ezpz_mc_quantiles_device.restype = C.c_int
    L.ezpz_mc_quantiles_device.argtypes = L.ezpz_mc_quantiles.argtypes + [vp]
    L.ezpz_system_tolerance_mc_quantiles.restype = C.c_int
    L.ezpz_system_tolerance_mc_quantiles.argtypes = L.ezpz_system_tolerance_mc.argtypes + [vp, sz, C.POINTER(CMcQuantileConfig), vp]
    L.ezpz_system_tolerance_mc_quantiles_device.restype = C.c_int
    L.ezpz_system_tolerance_mc_quantiles_device.argtypes = L.ezpz_system_tolerance_mc_quantiles.argtypes + [vp]
    L.ezpz_default_mc_effect_config.restype = None
    L.ezpz_default_mc_effect_config.argtypes = [C.POINTER(CMcEffectConfig)]
    L.ezpz_mc_effect_indices.restype = C.c_int
    L.ezpz_mc_effect_indices.argtypes = [vp, vp, vp, sz, sz, u32, vp, vp, vp, vp, vp]
    L.ezpz_mc_effects.restype = C.c_int
    L.ezpz_mc_effects.argtypes = [vp, vp, vp, vp, vp, vp, C.c_uint64, sz, sz, u32, u32, vp, vp]
    L.ezpz_mc_effects_device.restype = C.c_int
    L.ezpz_mc_effects_device.argtypes = L.ezpz_mc_effects.argtypes + [vp]
    L.ezpz_system_tolerance_mc_effects.restype = C.c_int
    L.ezpz_system_tolerance_mc_effects.argtypes = L.ezpz_system_tolerance_mc.argtypes + [C.POINTER(CMcEffectConfig)] + [vp] * 8
    L.ezpz_system_tolerance_mc_effects_device.restype = C.c_int
    L.ezpz_system_tolerance_mc_effects_device.argtypes = L.ezpz_system_tolerance_mc_effects.argtypes + [vp]
    L.ezpz_mc_factorial.restype = C.c_int
    L.ezpz_mc_factorial.argtypes = [vp, vp, vp, vp, u32, sz] + [vp] * 8
    L.ezpz_mc_factorial_device.restype = C.c_int
    L.ezpz_mc_factorial_device.argtypes = L.ezpz_mc_factorial.argtypes + [vp]
    L.ezpz_system_tolerance_mc_factorial.restype = C.c_int
    L.ezpz_system_tolerance_mc_factorial.argtypes = L.ezpz_system_tolerance_mc.argtypes + [vp] * 8
    L.ezpz_system_tolerance_mc_factorial_device.restype = C.c_int
    L.ezpz_system_tolerance_mc_factorial_device.argtypes = L.ezpz_system_tolerance_mc_factorial.argtypes + [vp]
    L.ezpz_sketch_image.restype = C.c_int
    L.ezpz_sketch_image.argtypes = [vp, vp, sz, sz, vp, sz, C.POINTER(CImageView), u32, C.c_int, vp, vp]
    L.ezpz_sketch_image_host.restype = C.c_int
    L.ezpz_sketch_image_host.argtypes = L.ezpz_sketch_image.argtypes
    L.ezpz_sketch_image_device.restype = C.c_int
    L.ezpz_sketch_image_device.argtypes = L.ezpz_sketch_image.argtypes + [vp]
    L.ezpz_sketch_compose.restype = C.c_int
    L.ezpz_sketch_compose.argtypes = [vp, C.POINTER(CImageView), u32, vp, vp, vp]
    L.ezpz_system_tolerance_mc_image.restype = C.c_int
    L.ezpz_system_tolerance_mc_image.argtypes = L.ezpz_system_tolerance_mc.argtypes + [vp, sz, C.POINTER(CImageView), u32, vp, vp]
    L.ezpz_system_tolerance_mc_image_device.restype = C.c_int
    L.ezpz_system_tolerance_mc_image_device.argtypes = L.ezpz_system_tolerance_mc_image.argtypes + [vp]
    L.ezpz_default_seek_config.argtypes = [C.POINTER(CSeekConfig)]
    L.ezpz_seek_step.restype = C.c_int
    L.ezpz_seek_step.argtypes = [sz, sz, vp, vp, vp, vp, C.POINTER(CSeekConfig), C.c_double, vp, vp, vp]
    L.ezpz_system_seek_targets.restype = C.c_int
    L.ezpz_system_seek_targets.argtypes = [vp, vp, vp, sz, vp, vp, sz, vp, sz, C.POINTER(CSeekConfig), vp, vp, vp, vp, vp]
    L.ezpz_system_seek_targets_device.restype = C.c_int
    L.ezpz_system_seek_targets_device.argtypes = L.ezpz_system_seek_targets.argtypes + [vp]
    L.ezpz_default_branch_config.restype = None
    L.ezpz_default_branch_config.argtypes = [C.POINTER(CBranchConfig)]
    L.ezpz_branch_cluster.restype = C.c_int
    L.ezpz_branch_cluster.argtypes = [vp, vp, vp, sz, C.c_uint64, sz, C.POINTER(CBranchConfig), vp, vp, vp, vp]
    L.ezpz_branch_cluster_device.restype = C.c_int
    L.ezpz_branch_cluster_device.argtypes = L.ezpz_branch_cluster.argtypes + [vp]
    L.ezpz_system_solve_branches.restype = C.c_int
    L.ezpz_system_solve_branches.argtypes = [vp, vp, vp, vp, sz, C.c_uint64, C.POINTER(CBranchConfig), C.POINTER(CConfig), vp, vp, vp, vp]
    L.ezpz_system_solve_branches_device.restype = C.c_int
    L.ezpz_system_solve_branches_device.argtypes = L.ezpz_system_solve_branches.argtypes + [vp]
    L.ezpz_current_device.restype = C.c_int
    L.ezpz_current_device.argtypes = []
    L.ezpz_host_register.restype = C.c_int
    L.ezpz_host_register.argtypes = [vp, sz]
    L.ezpz_host_unregister.restype = C.c_int
    L.ezpz_host_unregister.argtypes = [vp]
    L.ezpz_system_specialize.restype = C.c_int
    L.ezpz_system_specialize.argtypes = [vp, C.c_int]
    L.ezpz_specialized_source.restype = C.c_long
    L.ezpz_specialized_source.argtypes = [vp, sz, sz, C.c_int, C.c_char_p, sz]
    L.ezpz_multi_create.restype = C.c_int
    L.ezpz_multi_create.argtypes = [vp, sz, sz, C.c_uint64, u32, C.POINTER(vp), C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
    L.ezpz_multi_destroy.restype = None
    L.ezpz_multi_destroy.argtypes = [vp]
    L.ezpz_multi_device_count.restype = C.c_int
    L.ezpz_multi_device_count.argtypes = [vp]
    L.ezpz_multi_device.restype = C.c_int
    L.ezpz_multi_device.argtypes = [vp, C.c_int]
    L.ezpz_multi_shard.restype = None
    L.ezpz_multi_shard.argtypes = [vp, sz, C.c_int, C.POINTER(sz), C.POINTER(sz)]
    L.ezpz_multi_specialize.restype = C.c_int
    L.ezpz_multi_specialize.argtypes = [vp, C.c_int]
    L.ezpz_multi_solve_batch.restype = C.c_int
    L.ezpz_multi_solve_batch.argtypes = [vp, vp, sz, C.POINTER(CConfig), vp, vp, vp]
    L.ezpz_system_solve_batch_multi.restype = C.c_int
    L.ezpz_system_solve_batch_multi.argtypes = [vp, sz, sz, C.c_uint64, vp, sz, C.POINTER(CConfig), vp, vp]
    L.ezpz_resolve_sides.restype = C.c_int
    L.ezpz_resolve_sides.argtypes = [vp, sz, vp, sz]
    L.ezpz_mixed_create.restype = C.c_int
    L.ezpz_mixed_create.argtypes = [vp, sz, vp, sz, C.POINTER(vp)]
    L.ezpz_mixed_destroy.restype = None
    L.ezpz_mixed_destroy.argtypes = [vp]
    L.ezpz_mixed_total_values.restype = sz
    L.ezpz_mixed_total_values.argtypes = [vp]
    L.ezpz_mixed_offsets.restype = None
    L.ezpz_mixed_offsets.argtypes = [vp, vp]
    L.ezpz_mixed_solve_device.restype = C.c_int
    L.ezpz_mixed_solve_device.argtypes = [vp, vp, C.POINTER(CConfig), vp, vp, vp]
    L.ezpz_mixed_solve.restype = C.c_int
    L.ezpz_mixed_solve.argtypes = [vp, vp, C.POINTER(CConfig), vp, vp]
    L.ezpz_system_solve_batch_mixed.restype = C.c_int
    L.ezpz_system_solve_batch_mixed.argtypes = [vp, sz, vp, vp, sz, C.POINTER(CConfig), vp, vp]
    L.ezpz_multi_solve_batch_mixed.restype = C.c_int
    L.ezpz_multi_solve_batch_mixed.argtypes = [vp, sz, vp, vp, sz, C.POINTER(CConfig), vp, vp]
    L.ezpz_launch_policy.restype = C.c_int
    L.ezpz_launch_policy.argtypes = [C.c_int, C.POINTER(CLaunchPolicy)]
    L.ezpz_debug_call_trace.restype = sz
    L.ezpz_debug_call_trace.argtypes = [vp, sz]
    L.ezpz_debug_set_stamps.restype = None
    L.ezpz_debug_set_stamps.argtypes = [vp]
    L.ezpz_debug_freedom_exits.restype = None
    L.ezpz_debug_freedom_exits.argtypes = [vp]
    L.ezpz_debug_jit_compilations.restype = C.c_uint64
    L.ezpz_debug_jit_compilations.argtypes = []
    L.ezpz_debug_front_plan.restype = C.c_long
    L.ezpz_debug_front_plan.argtypes = [vp, sz, sz, u32, u32, C.c_uint64, vp, sz, vp]
    L.ezpz_cache_clear.restype = None
    L.ezpz_cache_clear.argtypes = []
    L.ezpz_analyze.restype = C.c_int
    L.ezpz_analyze.argtypes = [vp, sz, sz, C.POINTER(CSystemInfo), C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
    L.ezpz_system_eval_batch.restype = C.c_int
    L.ezpz_system_eval_batch.argtypes = [vp, vp, sz, vp, vp, vp]
    L.ezpz_system_residual_field.restype = C.c_int
    L.ezpz_system_residual_field.argtypes = [vp, vp, u32, u32, C.c_int64, C.POINTER(CViewport), vp, vp, C.POINTER(C.c_uint64)]
    L.ezpz_system_residual_field_device.restype = C.c_int
    L.ezpz_system_residual_field_device.argtypes = [vp, vp, u32, u32, C.c_int64, C.POINTER(CViewport), vp, vp, vp, vp]
    L.ezpz_residual_colormap.restype = None
    L.ezpz_residual_colormap.argtypes = [vp, sz, vp]
    L.ezpz_residual_overlay.restype = C.c_int
    L.ezpz_residual_overlay.argtypes = [vp, C.POINTER(CViewport), C.c_double, C.c_double, C.c_double, C.c_double]
    L.ezpz_system_jacobian_pattern.restype = C.c_int
    L.ezpz_system_jacobian_pattern.argtypes = [vp, vp, vp]
    L.ezpz_system_solve_batch_device.restype = C.c_int
    L.ezpz_system_solve_batch_device.argtypes = [vp, vp, sz, C.POINTER(CConfig), vp, vp, vp, vp, u32, vp]
    L.ezpz_system_solve_batch.restype = C.c_int
    L.ezpz_system_solve_batch.argtypes = [vp, vp, sz, C.POINTER(CConfig), vp, vp, vp, vp, u32]
    L.ezpz_constraint_has_param.restype = C.c_int
    L.ezpz_constraint_has_param.argtypes = [vp]
    L.ezpz_system_solve_batch_params_device.restype = C.c_int
    L.ezpz_system_solve_batch_params_device.argtypes = [vp, vp, vp, sz, vp, sz, C.POINTER(CConfig), vp, vp, vp, vp, u32, vp]
    L.ezpz_system_solve_batch_params.restype = C.c_int
    L.ezpz_system_solve_batch_params.argtypes = [vp, vp, vp, sz, vp, sz, C.POINTER(CConfig), vp, vp, vp, vp, u32]
    L.ezpz_constraint_param_derivative.restype = C.c_int
    L.ezpz_constraint_param_derivative.argtypes = [vp, vp, vp, C.POINTER(C.c_int)]
    L.ezpz_system_param_sensitivity_plan.restype = C.c_int
    L.ezpz_system_param_sensitivity_plan.argtypes = [vp, vp, sz, C.POINTER(CSensitivityPlan)]
    L.ezpz_system_param_sensitivity_device.restype = C.c_int
    L.ezpz_system_param_sensitivity_device.argtypes = [vp, vp, vp, sz, vp, sz, C.c_double, vp, vp, vp, vp]
    L.ezpz_system_param_sensitivity.restype = C.c_int
    L.ezpz_system_param_sensitivity.argtypes = [vp, vp, vp, sz, vp, sz, C.c_double, vp, vp, vp]
    L.ezpz_system_set_params_route.restype = C.c_int
    L.ezpz_system_set_params_route.argtypes = [vp, u32]
    L.ezpz_system_set_sensitivity_route.restype = C.c_int
    L.ezpz_system_set_sensitivity_route.argtypes = [vp, u32]
    L.ezpz_debug_front_sens_tables.restype = C.c_long
    L.ezpz_debug_front_sens_tables.argtypes = [vp, sz, sz, u32, u32, C.c_uint64, vp, sz, vp, sz, vp]
    L.ezpz_system_sweep_params_plan.restype = C.c_int
    L.ezpz_system_sweep_params_plan.argtypes = [vp, vp, sz, C.POINTER(CSweepPlan)]
    L.ezpz_system_sweep_params_device.restype = C.c_int
    L.ezpz_system_sweep_params_device.argtypes = [vp, vp, vp, sz, vp, sz, sz, C.POINTER(CConfig), vp, vp, vp, vp, u32, vp]
    L.ezpz_system_sweep_params.restype = C.c_int
    L.ezpz_system_sweep_params.argtypes = [vp, vp, vp, sz, vp, sz, sz, C.POINTER(CConfig), vp, vp, vp, vp, u32]
    L.ezpz_default_guard_config.restype = None
    L.ezpz_default_guard_config.argtypes = [C.POINTER(CGuardConfig)]
    L.ezpz_system_sweep_guarded_plan.restype = C.c_int
    L.ezpz_system_sweep_guarded_plan.argtypes = [vp, vp, sz, C.POINTER(CSweepPlan)]
    L.ezpz_system_sweep_guarded_device.restype = C.c_int
    L.ezpz_system_sweep_guarded_device.argtypes = [vp, vp, vp, sz, vp, vp, sz, sz, C.POINTER(CConfig), C.POINTER(CGuardConfig), vp, vp, vp,
                                                   vp, vp, vp, u32, vp]
    L.ezpz_system_sweep_guarded.restype = C.c_int
    L.ezpz_system_sweep_guarded.argtypes = [vp, vp, vp, sz, vp, vp, sz, sz, C.POINTER(CConfig), C.POINTER(CGuardConfig), vp, vp, vp, vp, vp,
                                            vp, u32]
    L.ezpz_solve_inner.restype = C.c_int
    L.ezpz_solve_inner.argtypes = [vp, vp, sz, vp, vp, sz, C.POINTER(CConfig), vp, vp, vp, sz, C.POINTER(COutcome)]
    L.ezpz_solve.restype = C.c_int
    L.ezpz_solve.argtypes = [vp, sz, vp, vp, sz, C.POINTER(CConfig), vp, vp, vp, sz, C.POINTER(COutcome)]
    L.ezpz_solve_analysis.restype = C.c_int
    L.ezpz_solve_analysis.argtypes = list(L.ezpz_solve.argtypes) + [vp, C.POINTER(C.c_uint64)]
    L.ezpz_problem_parse.restype = C.c_int
    L.ezpz_problem_parse.argtypes = [C.c_char_p, sz, C.POINTER(vp), C.c_char_p, sz]
    L.ezpz_problem_destroy.restype = None
    L.ezpz_problem_destroy.argtypes = [vp]
    L.ezpz_problem_num_constraints.restype = sz
    L.ezpz_problem_num_constraints.argtypes = [vp]
    L.ezpz_problem_num_vars.restype = sz
    L.ezpz_problem_num_vars.argtypes = [vp]
    L.ezpz_problem_constraints.restype = vp
    L.ezpz_problem_constraints.argtypes = [vp]
    L.ezpz_problem_guesses.restype = vp
    L.ezpz_problem_guesses.argtypes = [vp]
    L.ezpz_problem_num_labels.restype = sz
    L.ezpz_problem_num_labels.argtypes = [vp, C.c_int]
    L.ezpz_problem_label.restype = C.c_char_p
    L.ezpz_problem_label.argtypes = [vp, C.c_int, sz]
    L.ezpz_problem_num_lines.restype = sz
    L.ezpz_problem_num_lines.argtypes = [vp]
    L.ezpz_problem_line.restype = C.c_int
    L.ezpz_problem_line.argtypes = [vp, sz, C.POINTER(sz), C.POINTER(sz)]
    _lib = L
    return L
