"""ezpz_amd: the MI355X-native Newton / Levenberg-Marquardt constraint-solve path of KittyCAD/ezpz.

A C-ABI shared library (include/ezpz_amd.h; HIP kernels for gfx950 + C++ host symbolic phase) and this
thin host mirror of the `ezpz` crate's solve API.  There is no CPU fallback: importing works anywhere the
library builds, solving needs a HIP device.
"""
from . import residual_viz, textual
from ._lib import BRANCH_DTYPE, BRANCH_INFO_DTYPE, CONSTRAINT_DTYPE, GUARD_STEP_DTYPE, MC_DIST_DTYPE, MC_FACTORIAL_DTYPE, MC_MOMENTS_INFO_DTYPE, MC_QUANTILE_DTYPE, MC_STATS_DTYPE, MC_TOTALS_DTYPE, SEEK_INFO_DTYPE, SEEK_STATUS, STATUS_DTYPE, lib
from .api import (BranchConfig, BranchResult, cluster_branches, McDist, McResult, McContributors, mc_sample, mc_moments, mc_contributors, SobolIndices, SobolResult, mc_sobol_sums, mc_sobol_indices, mc_quantiles, EffectsConfig, McEffects, mc_effects, mc_effect_indices, mc_effect_edges, McFactorial, mc_factorial, mc_corner_count, SeekConfig, SeekResult, seek_step, Angle, AngleKind, CircleSide, Config, Constraint, ConstraintRequest, DatumCircle, DatumCircularArc,
                  DatumDistance, DatumLineSegment, DatumPoint, FailureOutcome, FreedomAnalysis, GuardConfig, IdGenerator, LineSide,
                  MixedBatch, MultiSystem, NonLinearSystemError, RawResult, RedundancyConfig, SolveOutcome, SolveOutcomeFreedomAnalysis, System, TEAM_AUTO_LATENCY, TEAM_AUTO_LISTS, TEAM_BATCH_LANES, TEAM_FRONTS, TEAM_LATENCY_PHASES, TEAM_LATENCY_RECORDS, TEAM_LATENCY_WAVE, Warning, WarningContent, analyze, constraint_has_param, constraint_measure, constraint_param_derivative, device_count, launch_policy, solve,
                  host_register, host_unregister, resolve_sides, solve_analysis, specialized_source, solve_batch, solve_batch_mixed, solve_batch_mixed_multi, solve_batch_multi, solve_records, stack_records)

from .sketch_image import (REFERENCE_LAYERS, ComposeLayer, DrawItem, ImageConfig, ImageInfo, ImageView, SketchImage, compose, fit_view, items_from_problem,
                           save_sketch_png, sketch_image, sketch_image_device, sketch_image_host)
from ._lib import DRAW_ITEM_DTYPE, IMAGE_INFO_DTYPE

__all__ = [
    "REFERENCE_LAYERS", "ComposeLayer", "DrawItem", "ImageConfig", "ImageInfo", "ImageView", "SketchImage", "compose", "fit_view", "items_from_problem",
    "save_sketch_png", "sketch_image", "sketch_image_device", "sketch_image_host", "DRAW_ITEM_DTYPE", "IMAGE_INFO_DTYPE",
    "Angle", "AngleKind", "CircleSide", "Config", "Constraint", "ConstraintRequest", "DatumCircle", "DatumCircularArc",
    "DatumDistance", "DatumLineSegment", "DatumPoint", "FailureOutcome", "FreedomAnalysis", "GuardConfig", "IdGenerator", "LineSide",
    "MixedBatch", "MultiSystem", "NonLinearSystemError", "RawResult", "RedundancyConfig", "SolveOutcome", "SolveOutcomeFreedomAnalysis", "System", "TEAM_AUTO_LATENCY", "TEAM_AUTO_LISTS", "TEAM_BATCH_LANES", "TEAM_FRONTS", "TEAM_LATENCY_PHASES", "TEAM_LATENCY_RECORDS", "TEAM_LATENCY_WAVE", "Warning", "WarningContent", "analyze", "constraint_has_param", "constraint_measure", "constraint_param_derivative",
    "device_count", "launch_policy", "host_register", "host_unregister", "resolve_sides", "solve", "specialized_source",
    "solve_analysis", "solve_batch", "solve_batch_mixed", "solve_batch_mixed_multi", "solve_batch_multi", "solve_records", "stack_records", "residual_viz", "textual", "lib", "CONSTRAINT_DTYPE", "GUARD_STEP_DTYPE", "STATUS_DTYPE",
    "McDist", "McResult", "McContributors", "mc_sample", "mc_moments", "mc_contributors", "SobolIndices", "SobolResult", "mc_sobol_sums", "mc_sobol_indices", "mc_quantiles", "EffectsConfig", "McEffects", "mc_effects", "mc_effect_indices", "mc_effect_edges", "McFactorial", "mc_factorial", "mc_corner_count", "MC_FACTORIAL_DTYPE", "MC_QUANTILE_DTYPE", "MC_DIST_DTYPE", "MC_MOMENTS_INFO_DTYPE", "MC_STATS_DTYPE", "MC_TOTALS_DTYPE",
    "SeekConfig", "SeekResult", "seek_step", "SEEK_INFO_DTYPE", "SEEK_STATUS",
    "BranchConfig", "BranchResult", "cluster_branches", "BRANCH_INFO_DTYPE", "BRANCH_DTYPE",
]
