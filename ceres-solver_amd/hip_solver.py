"""Python host side above the C ABI (include/ceres_hip.h).

Mirrors the reference's plugin interface for this path — same names, argument meaning
and error behaviour — so that the parity tests read like the reference's own tests:

    LinearSolverOptions   ~ ceres::internal::LinearSolver::Options         internal/ceres/linear_solver.h:148-230
    PerSolveOptions       ~ LinearSolver::PerSolveOptions                   internal/ceres/linear_solver.h:237-318
    Summary               ~ LinearSolver::Summary                           internal/ceres/linear_solver.h:320-326
    HipLinearSolver.solve ~ LinearSolver::Solve(A, b, per_solve_options, x) internal/ceres/linear_solver.h:339-342
    create_linear_solver  ~ LinearSolver::Create incl. its fall-backs        internal/ceres/linear_solver.cc:51-126

There is no CPU fall-back here: without libceres_hip.so or without a gfx950 device
every constructor raises.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, byref, c_char, c_char_p, c_double, c_int32, c_int64, c_uint8, c_uint32, c_void_p
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

from .block_structure import BlockStructure, CBlockStructure

# enum values equal the reference's (include/ceres/types.h:57-141, internal/ceres/linear_solver.h:57-74)
DENSE_SCHUR, ITERATIVE_SCHUR, CGNR = 3, 5, 6
IDENTITY, JACOBI, SCHUR_JACOBI, SCHUR_POWER_SERIES_EXPANSION, CLUSTER_JACOBI = 0, 1, 2, 3, 4
CANONICAL_VIEWS, SINGLE_LINKAGE = 0, 1   # ceres::VisibilityClusteringType (read with CLUSTER_JACOBI)
SUCCESS, NO_CONVERGENCE, FAILURE, FATAL_ERROR = 0, 1, 2, 3
PATH_GENERIC, PATH_BAL = 0, 1
E_INVALID, E_UNSUPPORTED, E_HIP, E_COMM, E_NODEVICE = -1, -2, -3, -4, -5   # CERES_HIP_E_* (include/ceres_hip.h)
TERMINATION_NAMES = {0: "SUCCESS", 1: "NO_CONVERGENCE", 2: "FAILURE", 3: "FATAL_ERROR"}
UNIQUE_ID_BYTES = 128
IPC_HANDLE_BYTES = 64

(TIMED_JTJX, TIMED_SX, TIMED_SCHUR_INIT, TIMED_SCHUR_JACOBI, TIMED_BACK_SUBSTITUTE, TIMED_PACK, TIMED_BLOCK_JACOBI, TIMED_COPY,
 TIMED_READ_STREAM, TIMED_CGNR_SETUP, TIMED_MODEL_COST, TIMED_JACOBIAN_GRAM, TIMED_CLUSTER_ELIMINATE, TIMED_CLUSTER_FACTOR,
 TIMED_CLUSTER_APPLY) = range(1, 16)

_HERE = os.path.dirname(os.path.abspath(__file__))


def library_path() -> str:
    # CERES_HIP_LIBRARY: an A/B build of the same sources (tools/build_variant.sh); never a different implementation
    return os.environ.get("CERES_HIP_LIBRARY") or os.path.join(_HERE, "csrc", "libceres_hip.so")


class COptions(ctypes.Structure):
    _fields_ = [("solver_type", c_int32), ("preconditioner_type", c_int32), ("min_num_iterations", c_int32),
                ("max_num_iterations", c_int32), ("residual_reset_period", c_int32), ("num_eliminate_blocks", c_int32),
                ("device", c_int32), ("force_generic_path", c_int32), ("cg_check_interval", c_int32),
                ("jacobian_storage", c_int32), ("max_num_spse_iterations", c_int32), ("use_spse_initialization", c_int32),
                ("spse_tolerance", c_double), ("use_explicit_schur_complement", c_int32), ("visibility_clustering_type", c_int32)]


class CSummary(ctypes.Structure):
    _fields_ = [("residual_norm", c_double), ("num_iterations", c_int32), ("termination_type", c_int32),
                ("message", c_char * 256)]


class CInfo(ctypes.Structure):
    _fields_ = [("kernel_path", c_int32), ("num_rows", c_int32), ("num_cols", c_int32), ("num_cols_e", c_int32),
                ("num_cols_f", c_int32), ("num_row_blocks_e", c_int32), ("num_e_blocks", c_int32),
                ("num_f_blocks", c_int32), ("row_block_size", c_int32), ("e_block_size", c_int32),
                ("f_block_size", c_int32), ("num_nonzeros", c_int64), ("num_observations", c_int64),
                ("num_tiles", c_int64), ("device_bytes", c_int64), ("camera_accum_in_lds", c_int32),
                ("world_size", c_int32), ("rank", c_int32), ("p2p_enabled", c_int32), ("p2p_fine_grained", c_int32),
                ("camera_accum_hybrid", c_int32), ("hybrid_popular_rows", c_int32), ("num_observations_in_lds", c_int64),
                ("points_renumbered", c_int32), ("cg_iteration_in_operator", c_int32), ("collectives_last_step", c_int32)]


class CTiming(ctypes.Structure):
    _fields_ = [("upload_ms", c_double), ("pack_ms", c_double), ("setup_ms", c_double), ("preconditioner_ms", c_double),
                ("cg_ms", c_double), ("back_substitute_ms", c_double), ("download_ms", c_double), ("total_ms", c_double),
                ("operator_applications", c_int32), ("reserved", c_int32)]


class CLmOptions(ctypes.Structure):
    _fields_ = [("radius", c_double), ("min_diagonal", c_double), ("max_diagonal", c_double), ("eta", c_double),
                ("reuse_diagonal", c_int32), ("values_unchanged", c_int32)]


class CLmResult(ctypes.Structure):
    _fields_ = [("linear_solver", CSummary), ("model_cost_change", c_double), ("step_is_finite", c_int32),
                ("reserved", c_int32)]


# every symbol include/ceres_hip.h declares: (name, restype, argtypes)
_DP = POINTER(c_double)
ABI_VERSION = 2   # CERES_HIP_ABI_VERSION of include/ceres_hip.h this binding mirrors (struct layouts below)

ABI = [
    ("ceres_hip_abi_version", c_int32, []),
    ("ceres_hip_device_count", c_int32, []),
    ("ceres_hip_create", c_void_p, [POINTER(COptions)]),
    ("ceres_hip_destroy", None, [c_void_p]),
    ("ceres_hip_last_error", c_char_p, [c_void_p]),
    ("ceres_hip_set_structure", c_int32, [c_void_p, POINTER(CBlockStructure)]),
    ("ceres_hip_get_info", c_int32, [c_void_p, POINTER(CInfo)]),
    ("ceres_hip_comm_get_unique_id", c_int32, [POINTER(c_uint8)]),
    ("ceres_hip_comm_init", c_int32, [c_void_p, POINTER(c_uint8), c_int32, c_int32]),
    ("ceres_hip_comm_p2p_prepare", c_int32, [c_void_p, c_int32, c_int32, c_int64, POINTER(c_uint8)]),
    ("ceres_hip_comm_p2p_connect", c_int32, [c_void_p, POINTER(c_uint8)]),
    ("ceres_hip_comm_p2p_selftest", c_int32, [c_void_p]),
    ("ceres_hip_comm_p2p_disable", c_int32, [c_void_p]),
    ("ceres_hip_debug_allreduce_timing", c_int32, [c_void_p, c_int64, c_int32, _DP]),
    ("ceres_hip_debug_last_backsub_route", c_int32, [c_void_p]),
    ("ceres_hip_solve", c_int32, [c_void_p, _DP, _DP, _DP, c_double, c_double, _DP, POINTER(CSummary)]),
    ("ceres_hip_solve_device", c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_double, c_double, c_void_p, POINTER(CSummary)]),
    ("ceres_hip_solve_unchanged_values", c_int32, [c_void_p, _DP, c_double, c_double, _DP, POINTER(CSummary)]),
    ("ceres_hip_load", c_int32, [c_void_p, _DP, _DP, _DP]),
    ("ceres_hip_load_device", c_int32, [c_void_p, c_void_p, c_void_p, c_void_p]),
    ("ceres_hip_op_right_multiply", c_int32, [c_void_p, _DP, _DP]),
    ("ceres_hip_op_left_multiply", c_int32, [c_void_p, _DP, _DP]),
    ("ceres_hip_op_right_multiply_e", c_int32, [c_void_p, _DP, _DP]),
    ("ceres_hip_op_right_multiply_f", c_int32, [c_void_p, _DP, _DP]),
    ("ceres_hip_op_left_multiply_e", c_int32, [c_void_p, _DP, _DP]),
    ("ceres_hip_op_left_multiply_f", c_int32, [c_void_p, _DP, _DP]),
    ("ceres_hip_op_block_diagonal_ete", c_int32, [c_void_p, _DP, c_int64]),
    ("ceres_hip_op_block_diagonal_ftf", c_int32, [c_void_p, _DP, c_int64]),
    ("ceres_hip_op_squared_column_norm", c_int32, [c_void_p, _DP]),
    ("ceres_hip_op_jtjx", c_int32, [c_void_p, _DP, _DP]),
    ("ceres_hip_op_jtb", c_int32, [c_void_p, _DP]),
    ("ceres_hip_op_jacobian_gram", c_int32, [c_void_p, _DP, _DP, _DP]),
    ("ceres_hip_op_schur_init", c_int32, [c_void_p]),
    ("ceres_hip_get_schur_rhs", c_int32, [c_void_p, _DP]),
    ("ceres_hip_get_ete_inverse", c_int32, [c_void_p, _DP, c_int64]),
    ("ceres_hip_op_schur_sx", c_int32, [c_void_p, _DP, _DP]),
    ("ceres_hip_op_back_substitute", c_int32, [c_void_p, _DP, _DP]),
    ("ceres_hip_op_power_series_operator", c_int32, [c_void_p, _DP, _DP]),
    ("ceres_hip_op_spse_apply", c_int32, [c_void_p, _DP, _DP, c_int32, c_double]),
    ("ceres_hip_op_block_jacobi_update", c_int32, [c_void_p]),
    ("ceres_hip_op_schur_jacobi_update", c_int32, [c_void_p]),
    ("ceres_hip_op_cluster_jacobi_update", c_int32, [c_void_p]),
    ("ceres_hip_cluster_jacobi_stats", c_int32, [c_void_p, POINTER(c_int32), POINTER(c_int32), POINTER(c_int64), _DP]),
    ("ceres_hip_debug_cluster_cameras", c_int32, [POINTER(CBlockStructure), c_int32, c_int32, POINTER(c_int32), POINTER(c_int32)]),
    ("ceres_hip_get_preconditioner_blocks", c_int32, [c_void_p, c_int32, _DP, c_int64]),
    ("ceres_hip_op_precond_apply", c_int32, [c_void_p, _DP, _DP]),
    ("ceres_hip_op_schur_eliminate_dense", c_int32, [c_void_p, _DP, _DP]),
    ("ceres_hip_schur_storage_info", c_int32, [c_void_p, POINTER(c_int64), POINTER(c_int64)]),
    ("ceres_hip_op_schur_eliminate_sparse", c_int32, [c_void_p, POINTER(c_int32), POINTER(c_int32), POINTER(c_int64), _DP, c_int64, c_int64]),
    ("ceres_hip_op_schur_symmetric_multiply", c_int32, [c_void_p, _DP, _DP]),
    ("ceres_hip_op_eliminator_back_substitute", c_int32, [c_void_p, _DP, _DP]),
    ("ceres_hip_op_dot", c_int32, [c_void_p, _DP, _DP, c_int64, _DP]),
    ("ceres_hip_op_axpby", c_int32, [c_void_p, c_double, _DP, c_double, _DP, c_int64, _DP]),
    ("ceres_hip_lm_compute_step", c_int32, [c_void_p, _DP, _DP, POINTER(CLmOptions), _DP, POINTER(CLmResult)]),
    ("ceres_hip_lm_compute_step_device", c_int32, [c_void_p, c_void_p, c_void_p, POINTER(CLmOptions), c_void_p, POINTER(CLmResult)]),
    ("ceres_hip_get_lm_diagonal", c_int32, [c_void_p, _DP]),
    ("ceres_hip_values_begin", c_int32, [c_void_p, _DP, _DP]),
    ("ceres_hip_values_ready", c_int32, [c_void_p, c_int32, c_int32]),
    ("ceres_hip_values_end", c_int32, [c_void_p, _DP]),
    ("ceres_hip_get_stream_stats", c_int32, [c_void_p, POINTER(c_int64), POINTER(c_int64), POINTER(c_int32)]),
    ("ceres_hip_debug_value_streams", c_int32, [POINTER(CBlockStructure), POINTER(c_int32), POINTER(c_int64), POINTER(c_int64)]),
    ("ceres_hip_debug_read_loaded", c_int32, [c_void_p, _DP, _DP]),
    ("ceres_hip_op_scale_columns", c_int32, [c_void_p, _DP, _DP]),
    ("ceres_hip_time_op", c_int32, [c_void_p, c_int32, c_int32, _DP]),
    ("ceres_hip_get_last_timing", c_int32, [c_void_p, POINTER(CTiming)]),
    ("ceres_hip_set_phase_timing", c_int32, [c_void_p, c_int32]),
    ("ceres_hip_debug_comm_loopback", c_int32, [c_void_p, c_int32]),
    ("ceres_hip_debug_comm_ghost_peers", c_int32, [c_void_p, c_int32, c_int64]),
    ("ceres_hip_debug_plan", c_int32, [POINTER(CBlockStructure), c_int32, POINTER(c_int32), POINTER(c_int64),
                                       POINTER(c_int32), POINTER(c_int32), POINTER(c_int32), POINTER(c_uint32),
                                       POINTER(c_int32), POINTER(c_int32), c_int64, c_char_p, c_int32]),
    ("ceres_hip_op_dense_cholesky_solve", c_int32, [c_void_p, c_int32, _DP, _DP, _DP, c_int32, POINTER(c_double), POINTER(c_int32)]),
    ("ceres_hip_op_dense_cholesky_factor", c_int32, [c_void_p, c_int32, _DP, _DP, _DP, _DP, c_int32, POINTER(c_int32), POINTER(c_int64),
                                                     POINTER(c_int32)]),
    ("ceres_hip_debug_hybrid_plan", c_int32, [POINTER(CBlockStructure), c_int32, c_int32, c_int32, POINTER(c_int64)] + [POINTER(c_int32)] * 8 +
     [c_int64, c_int64, c_int64]),
    ("ceres_hip_debug_staged_x_plan", c_int32, [POINTER(CBlockStructure), c_int32, POINTER(c_int64), POINTER(c_int32), POINTER(c_int32), c_int64, c_int64]),
    ("ceres_hip_debug_long_rounds", c_int32, [POINTER(CBlockStructure), c_int32, c_int32, c_int32, c_int32, POINTER(c_int64)] +
     [POINTER(c_int32)] * 7 + [POINTER(c_uint32), c_int64, c_int64, c_int64]),
]

_lib = None


class CMinimizerOptions(ctypes.Structure):
    _fields_ = [("max_num_iterations", c_int32), ("jacobi_scaling", c_int32), ("max_consecutive_invalid_steps", c_int32),
                ("reserved", c_int32), ("initial_trust_region_radius", c_double), ("max_trust_region_radius", c_double),
                ("min_trust_region_radius", c_double), ("min_lm_diagonal", c_double), ("max_lm_diagonal", c_double),
                ("min_relative_decrease", c_double), ("eta", c_double), ("function_tolerance", c_double),
                ("gradient_tolerance", c_double), ("parameter_tolerance", c_double)]


class CIterationSummary(ctypes.Structure):
    _fields_ = [("cost", c_double), ("cost_change", c_double), ("gradient_max_norm", c_double), ("step_norm", c_double),
                ("relative_decrease", c_double), ("trust_region_radius", c_double), ("step_is_successful", c_int32),
                ("step_is_valid", c_int32), ("linear_solver_iterations", c_int32), ("linear_solver_termination", c_int32)]


MAX_LOGGED_ITERATIONS = 256


class CMinimizerSummary(ctypes.Structure):
    _fields_ = [("initial_cost", c_double), ("final_cost", c_double), ("num_successful_steps", c_int32),
                ("num_unsuccessful_steps", c_int32), ("num_linear_solves", c_int32), ("termination_type", c_int32),
                ("linear_solver_seconds", c_double), ("evaluation_seconds", c_double), ("total_seconds", c_double),
                ("num_iterations_logged", c_int32), ("reserved", c_int32),
                ("iterations", CIterationSummary * MAX_LOGGED_ITERATIONS), ("message", ctypes.c_char * 256)]


ABI += [
    ("ceres_hip_bal_create", c_void_p, [POINTER(COptions), c_int32, c_int32, c_int64, POINTER(c_int32), POINTER(c_int32), _DP]),
    ("ceres_hip_bal_create_with_camera", c_void_p, [POINTER(COptions), c_int32, c_int32, c_int32, c_int64, POINTER(c_int32),
                                                    POINTER(c_int32), _DP]),
    ("ceres_hip_bal_create_with_constant_blocks", c_void_p, [POINTER(COptions), c_int32, c_int32, c_int32, c_int64, POINTER(c_int32),
                                                             POINTER(c_int32), _DP, POINTER(ctypes.c_uint8), POINTER(ctypes.c_uint8)]),
    ("ceres_hip_bal_create_with_fixed_intrinsics", c_void_p, [POINTER(COptions), c_int32, c_int32, c_int32, c_int64, POINTER(c_int32),
                                                              POINTER(c_int32), _DP, POINTER(ctypes.c_uint8), POINTER(ctypes.c_uint8),
                                                              POINTER(ctypes.c_uint8)]),
    ("ceres_hip_bal_create_with_shared_intrinsics", c_void_p, [POINTER(COptions), c_int32, c_int32, c_int32, c_int64, POINTER(c_int32),
                                                               POINTER(c_int32), _DP, POINTER(ctypes.c_uint8), POINTER(c_int32), c_int32]),
    ("ceres_hip_bal_reduced_sizes", c_int32, [c_void_p, POINTER(c_int64), POINTER(c_int64), POINTER(c_int64), POINTER(c_int32),
                                              POINTER(c_int32)]),
    ("ceres_hip_bal_fixed_cost", c_int32, [c_void_p, _DP, _DP]),
    ("ceres_hip_debug_bal_reduce", c_int32, [c_int32, c_int32, c_int64, POINTER(c_int32), POINTER(c_int32), POINTER(ctypes.c_uint8),
                                             POINTER(ctypes.c_uint8), POINTER(c_int64), POINTER(c_int64), POINTER(c_int32),
                                             POINTER(c_int32), POINTER(c_int32)]),
    ("ceres_hip_bal_num_effective_parameters", c_int32, [c_void_p, POINTER(c_int64)]),
    ("ceres_hip_bal_destroy", None, [c_void_p]),
    ("ceres_hip_bal_last_error", c_char_p, [c_void_p]),
    ("ceres_hip_bal_linear_solver", c_void_p, [c_void_p]),
    ("ceres_hip_debug_bal_evaluate_tiles_timing", c_int32, [c_void_p, _DP, c_int32, c_int32, _DP]),
    ("ceres_hip_bal_sizes", c_int32, [c_void_p, POINTER(c_int64), POINTER(c_int64), POINTER(c_int64)]),
    ("ceres_hip_bal_get_row_order", c_int32, [c_void_p, POINTER(c_int32)]),
    ("ceres_hip_bal_set_loss", c_int32, [c_void_p, c_int32, c_double, c_double, c_double]),
    ("ceres_hip_bal_set_inner_iterations", c_int32, [c_void_p, c_int32, c_double]),
    ("ceres_hip_bal_inner_iterate", c_int32, [c_void_p, _DP, _DP, _DP, POINTER(c_int32)]),
    ("ceres_hip_bal_inner_iteration_stats", c_int32, [c_void_p, POINTER(c_int32), _DP, POINTER(c_int32)]),
    ("ceres_hip_bal_set_trust_region_strategy", c_int32, [c_void_p, c_int32, c_int32]),
    ("ceres_hip_debug_dogleg_subspace_minimum", c_int32, [_DP, _DP, c_double, _DP]),
    ("ceres_hip_debug_inner_iteration_ordering", c_int32, [c_int32, c_int32, c_int64, POINTER(c_int32), POINTER(c_int32), c_int32,
                                                           POINTER(c_int32), POINTER(c_int32)]),
    ("ceres_hip_bal_evaluate", c_int32, [c_void_p, _DP, _DP, _DP, _DP, _DP]),
    ("ceres_hip_minimizer_default_options", None, [POINTER(CMinimizerOptions)]),
    ("ceres_hip_bal_minimize", c_int32, [c_void_p, POINTER(CMinimizerOptions), _DP, POINTER(CMinimizerSummary)]),
]


# ---- the line search minimizer (include/ceres_hip.h: ceres_hip_line_search_*) ----
STEEPEST_DESCENT, NONLINEAR_CONJUGATE_GRADIENT, LBFGS, BFGS = 0, 1, 2, 3
FLETCHER_REEVES, POLAK_RIBIERE, HESTENES_STIEFEL = 0, 1, 2
ARMIJO, WOLFE = 0, 1
BISECTION, QUADRATIC, CUBIC = 0, 1, 2


class CLineSearchOptions(ctypes.Structure):
    _fields_ = [("max_num_iterations", c_int32), ("line_search_direction_type", c_int32), ("nonlinear_conjugate_gradient_type", c_int32),
                ("max_lbfgs_rank", c_int32), ("use_approximate_eigenvalue_bfgs_scaling", c_int32), ("line_search_type", c_int32),
                ("line_search_interpolation_type", c_int32), ("max_num_line_search_step_size_iterations", c_int32),
                ("max_num_line_search_direction_restarts", c_int32), ("reserved", c_int32), ("min_line_search_step_size", c_double),
                ("line_search_sufficient_function_decrease", c_double), ("max_line_search_step_contraction", c_double),
                ("min_line_search_step_contraction", c_double), ("line_search_sufficient_curvature_decrease", c_double),
                ("max_line_search_step_expansion", c_double), ("function_tolerance", c_double), ("gradient_tolerance", c_double),
                ("parameter_tolerance", c_double)]


class CLineSearchIteration(ctypes.Structure):
    _fields_ = [("cost", c_double), ("cost_change", c_double), ("gradient_max_norm", c_double), ("gradient_norm", c_double),
                ("step_norm", c_double), ("step_size", c_double), ("line_search_function_evaluations", c_int32),
                ("line_search_gradient_evaluations", c_int32), ("line_search_iterations", c_int32), ("reserved", c_int32)]


class CLineSearchSummary(ctypes.Structure):
    _fields_ = [("initial_cost", c_double), ("final_cost", c_double), ("num_iterations", c_int32), ("num_successful_steps", c_int32),
                ("num_line_search_steps", c_int32), ("num_line_search_direction_restarts", c_int32), ("num_function_evaluations", c_int32),
                ("num_gradient_evaluations", c_int32), ("termination_type", c_int32), ("num_iterations_logged", c_int32),
                ("evaluation_seconds", c_double), ("direction_seconds", c_double), ("total_seconds", c_double),
                ("lbfgs_history_bytes", c_int64), ("iterations", CLineSearchIteration * MAX_LOGGED_ITERATIONS),
                ("message", ctypes.c_char * 256)]


class CLineSearchResult(ctypes.Structure):
    _fields_ = [("success", c_int32), ("num_function_evaluations", c_int32), ("num_gradient_evaluations", c_int32),
                ("num_iterations", c_int32), ("optimal_step_size", c_double), ("optimal_value", c_double), ("error", ctypes.c_char * 512)]


UNIVARIATE_FN = ctypes.CFUNCTYPE(c_int32, c_double, c_int32, _DP, _DP, c_void_p)

ABI += [
    ("ceres_hip_line_search_default_options", None, [POINTER(CLineSearchOptions)]),
    ("ceres_hip_bal_evaluate_gradient", c_int32, [c_void_p, _DP, _DP, _DP]),
    ("ceres_hip_bal_minimize_line_search", c_int32, [c_void_p, POINTER(CLineSearchOptions), _DP, POINTER(CLineSearchSummary)]),
    # (the callback — a UNIVARIATE_FN — travels as a plain pointer, so that NULL can be passed like every other pointer)
    ("ceres_hip_debug_line_search", c_int32, [POINTER(CLineSearchOptions), c_void_p, c_void_p, c_double, c_double, c_double,
                                              POINTER(CLineSearchResult)]),
    ("ceres_hip_debug_minimize_interpolating_polynomial", c_int32, [c_int32, _DP, _DP, POINTER(c_int32), _DP, POINTER(c_int32), c_double,
                                                                    c_double, _DP, _DP, _DP]),
    ("ceres_hip_debug_lbfgs_direction", c_int32, [c_int64, c_int32, c_int32, c_int32, _DP, _DP, _DP, _DP, POINTER(c_int32)]),
]


# ---- covariance (include/ceres_hip.h: ceres_hip_bal_covariance; design/17_covariance.md) ----
class CCovarianceOptions(ctypes.Structure):
    _fields_ = [("apply_loss_function", c_int32), ("reserved", c_int32), ("min_scaled_pivot", c_double)]


class CCovarianceSummary(ctypes.Structure):
    _fields_ = [("termination_type", c_int32), ("reserved", c_int32), ("min_point_pivot", c_double), ("min_schur_pivot", c_double),
                ("evaluate_seconds", c_double), ("eliminate_seconds", c_double), ("factor_seconds", c_double),
                ("inverse_seconds", c_double), ("blocks_seconds", c_double), ("device_bytes", c_int64), ("message", ctypes.c_char * 256)]


ABI += [
    ("ceres_hip_covariance_default_options", None, [POINTER(CCovarianceOptions)]),
    ("ceres_hip_bal_covariance", c_int32, [c_void_p, POINTER(CCovarianceOptions), _DP, c_int64, POINTER(c_int32), POINTER(c_int32), _DP,
                                           POINTER(CCovarianceSummary)]),
]


# ---- bound constraints (include/ceres_hip.h: ceres_hip_bal_set_bounds; design/23_bounds.md) ----
ABI += [
    ("ceres_hip_bal_set_bounds", c_int32, [c_void_p, _DP, _DP, POINTER(CLineSearchOptions)]),
    ("ceres_hip_bal_project", c_int32, [c_void_p, _DP, POINTER(c_int64)]),
    ("ceres_hip_bal_bounds_stats", c_int32, [c_void_p, POINTER(c_int32), POINTER(c_int32), POINTER(c_int32), POINTER(c_int32), _DP,
                                             POINTER(c_int64), POINTER(c_int32), POINTER(c_int32), _DP]),
    ("ceres_hip_debug_bal_bounded_step", c_int32, [c_void_p, _DP, _DP, c_double, _DP, _DP, _DP, _DP]),
]


def load_library():
    """dlopen csrc/libceres_hip.so and bind every ABI symbol; raises if anything is missing."""
    global _lib
    if _lib is None:
        # PyTorch-ROCm wheels bundle their own libamdhip64 / libhsa-runtime64 / librccl (same
        # SONAMEs as /opt/rocm's).  Two HIP runtimes in one process cannot both own the GPU, so
        # if torch is going to be used in this process it must be loaded FIRST; our library's
        # NEEDED entries then bind to the copies torch already mapped.
        import sys
        if "torch" not in sys.modules and os.environ.get("CERES_HIP_NO_TORCH", "0") != "1":
            try:
                import torch  # noqa: F401
            except Exception:
                pass
        path = library_path()
        if not os.path.exists(path):
            raise RuntimeError(f"{path} is missing: run `python __graft_entry__.py` (build()) first; "
                               "there is no fall-back implementation")
        lib = ctypes.CDLL(path)
        for name, restype, argtypes in ABI:
            fn = getattr(lib, name)  # AttributeError if the symbol is not exported
            fn.restype = restype
            fn.argtypes = argtypes
        if lib.ceres_hip_abi_version() != ABI_VERSION:
            raise RuntimeError(f"ABI version mismatch: the library says {lib.ceres_hip_abi_version()}, this binding is written for {ABI_VERSION}")
        _lib = lib
    return _lib


def device_count() -> int:
    return int(load_library().ceres_hip_device_count())


class HipError(RuntimeError):
    pass


@dataclass
class LinearSolverOptions:
    """LinearSolver::Options (internal/ceres/linear_solver.h:148-230), the fields this path reads."""
    type: int = ITERATIVE_SCHUR
    preconditioner_type: int = JACOBI
    min_num_iterations: int = 1          # reference default
    max_num_iterations: int = 1          # reference default (!); callers set it
    residual_reset_period: int = 10
    elimination_groups: List[int] = field(default_factory=list)
    # device-side knobs (not in the reference)
    device: int = 0
    force_generic_path: bool = False
    cg_check_interval: int = 0
    jacobian_storage: int = 0   # 1: fp32 tiles on the <2,3,9> path (accuracy mode, not parity)
    max_num_spse_iterations: int = 5
    use_spse_initialization: bool = False
    spse_tolerance: float = 0.1
    use_explicit_schur_complement: bool = False   # ITERATIVE_SCHUR on an explicitly formed (dense) S; SCHUR_JACOBI only
    visibility_clustering_type: int = CANONICAL_VIEWS   # CLUSTER_JACOBI: CANONICAL_VIEWS or SINGLE_LINKAGE (Preconditioner::Options)


@dataclass
class PerSolveOptions:
    """LinearSolver::PerSolveOptions (internal/ceres/linear_solver.h:237-318)."""
    D: Optional[np.ndarray] = None
    q_tolerance: float = 0.0
    r_tolerance: float = 0.0


@dataclass
class Summary:
    residual_norm: float = -1.0
    num_iterations: int = -1
    termination_type: int = FAILURE
    message: str = ""

    @property
    def termination_name(self):
        return TERMINATION_NAMES.get(self.termination_type, "?")


def _f64(a, n=None, name="array"):
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=np.float64)
    if n is not None and a.shape[0] < n:
        raise ValueError(f"{name} has {a.shape[0]} elements, need {n}")
    return a


def _p(a):
    return None if a is None else a.ctypes.data_as(_DP)


class HipLinearSolver:
    """One device-resident solver instance = one ceres::internal::LinearSolver object.

    The structure is set once (the reference guarantees constant sparsity per instance,
    internal/ceres/linear_solver.h:137-142); each `solve` uploads values / b / D and returns x.
    """

    def __init__(self, options: LinearSolverOptions, comm_id: Optional[bytes] = None, rank: int = 0,
                 world_size: int = 1, loopback_world: int = 0, p2p_exchange=None, p2p_max_elements: int = 0, ghost_world: int = 0):
        """comm_id: RCCL unique id (ceres_hip_comm_init).  p2p_exchange: callable(bytes) -> list of every rank's bytes in
        rank order (e.g. a torch.distributed all_gather); connects the one-shot peer-to-peer all-reduce for vectors of
        up to p2p_max_elements doubles (99 * number of F blocks covers a step: blocks, rhs and column norms go through ONE all-reduce)."""
        self._lib = load_library()
        self.options = options
        nelim = options.elimination_groups[0] if options.elimination_groups else 0
        c = COptions(options.type, options.preconditioner_type, options.min_num_iterations,
                     options.max_num_iterations, options.residual_reset_period, nelim, options.device,
                     int(options.force_generic_path), options.cg_check_interval, options.jacobian_storage,
                     options.max_num_spse_iterations, int(options.use_spse_initialization), options.spse_tolerance,
                     int(options.use_explicit_schur_complement), int(options.visibility_clustering_type))
        self._h = self._lib.ceres_hip_create(byref(c))
        if not self._h:
            raise HipError(self._lib.ceres_hip_last_error(None).decode())
        self.bs = None
        self._values_extent = None
        if world_size > 1 and comm_id is not None:
            buf = (c_uint8 * UNIQUE_ID_BYTES).from_buffer_copy(comm_id)
            self._check(self._lib.ceres_hip_comm_init(self._h, buf, rank, world_size))
        self.p2p_ok = False
        self.p2p_error = ""
        if world_size > 1 and p2p_exchange is not None:
            # every step is collective: a rank that fails still takes part in the exchange, and reports through p2p_ok
            mine = (c_uint8 * IPC_HANDLE_BYTES)()
            ok = self._lib.ceres_hip_comm_p2p_prepare(self._h, rank, world_size, int(p2p_max_elements), mine) == 0
            if not ok:
                self.p2p_error = self._lib.ceres_hip_last_error(self._h).decode()
            handles = p2p_exchange(bytes(mine))
            if len(handles) != world_size or any(len(h) != IPC_HANDLE_BYTES for h in handles):
                raise HipError("p2p_exchange must return one 64-byte handle per rank")
            if ok:
                allh = (c_uint8 * (IPC_HANDLE_BYTES * world_size)).from_buffer_copy(b"".join(handles))
                ok = self._lib.ceres_hip_comm_p2p_connect(self._h, allh) == 0
                if not ok:
                    self.p2p_error = self._lib.ceres_hip_last_error(self._h).decode()
            self.p2p_ok = ok
            if not ok and comm_id is None:
                raise HipError("peer-to-peer communicator failed and there is no RCCL communicator: " + self.p2p_error)
        if loopback_world > 1:  # debug: sharded code paths on one GPU (see include/ceres_hip.h)
            self._check(self._lib.ceres_hip_debug_comm_loopback(self._h, loopback_world))
        if ghost_world > 1:  # measurement: rank 0 of ghost_world ranks, the peers are local dummy buffers (include/ceres_hip.h)
            self._check(self._lib.ceres_hip_debug_comm_ghost_peers(self._h, ghost_world, int(p2p_max_elements)))
            self.p2p_ok = True

    def p2p_selftest(self) -> bool:
        """Collective: all-reduces of known values through the peer-to-peer path.  ceres_hip_comm_p2p_connect has already run it once
        (the path is never enabled untested); this repeats it on request."""
        if not self.p2p_ok:
            return False
        rc = self._lib.ceres_hip_comm_p2p_selftest(self._h)
        if rc != 0:
            self.p2p_error = self._lib.ceres_hip_last_error(self._h).decode()
            self.p2p_ok = False
        return rc == 0

    def allreduce_timing(self, n: int, iters: int = 200) -> float:
        """Collective: average microseconds per all-reduce of n doubles (measurement helper)."""
        out = np.zeros(1)
        self._check(self._lib.ceres_hip_debug_allreduce_timing(self._h, int(n), int(iters), _p(out)))
        return float(out[0])

    def last_backsub_route(self) -> int:
        """ceres_hip_debug_last_backsub_route: 0 = the last ITERATIVE_SCHUR solve back-substituted over J, 1 = it took the point tail."""
        return int(self._lib.ceres_hip_debug_last_backsub_route(self._h))

    def p2p_disable(self):
        self._check(self._lib.ceres_hip_comm_p2p_disable(self._h))
        self.p2p_ok = False

    # -- plumbing ----------------------------------------------------------
    def _check(self, rc):
        if rc != 0:
            raise HipError(f"ceres_hip error {rc}: {self._lib.ceres_hip_last_error(self._h).decode()}")

    def _check_not_streaming(self, rc):
        """The solve entries report a failure as a FATAL_ERROR summary, like a LinearSolver that could not run; a call the library
        refused because a streamed upload is open (values_begin without values_end) is the caller's mistake and raises like the others."""
        if rc != 0 and getattr(self, "_stream_keep", None) is not None:
            self._check(rc)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.ceres_hip_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- structure ---------------------------------------------------------
    def set_structure(self, bs: BlockStructure):
        self.bs = bs
        self._cbs = bs.as_ctypes()
        self._check(self._lib.ceres_hip_set_structure(self._h, byref(self._cbs)))
        self._info = self.info()
        self._values_extent = bs.values_extent()  # O(num_cells) to compute: once, not per solve

    def info(self) -> CInfo:
        i = CInfo()
        self._check(self._lib.ceres_hip_get_info(self._h, byref(i)))
        return i

    # -- the boundary call -------------------------------------------------
    def solve(self, values, b, per_solve_options: PerSolveOptions = PerSolveOptions()):
        """LinearSolver::Solve.  Returns (x, Summary).  x is pre-poisoned with NaN like the
        caller does (internal/ceres/levenberg_marquardt_strategy.cc:110)."""
        n = self._info
        values = _f64(values, self._values_extent, "values")
        b = _f64(b, n.num_rows, "b")
        D = _f64(per_solve_options.D, n.num_cols, "D")
        x = np.full(n.num_cols, np.nan)
        s = CSummary()
        rc = self._lib.ceres_hip_solve(self._h, _p(values), _p(b), _p(D), per_solve_options.q_tolerance,
                                       per_solve_options.r_tolerance, _p(x), byref(s))
        self._check_not_streaming(rc)
        summary = Summary(s.residual_norm, s.num_iterations, s.termination_type, s.message.decode(errors="replace"))
        if rc != 0:
            summary.termination_type = FATAL_ERROR
            summary.message = self._lib.ceres_hip_last_error(self._h).decode()
        return x, summary

    def solve_unchanged_values(self, per_solve: "PerSolveOptions"):
        """LinearSolver::Solve again on the values and b of the previous solve() / load() with a new D (the retry after a rejected
        trust-region step): only D crosses PCIe, the tiles are not rebuilt."""
        n = self._info
        D = None if per_solve.D is None else _f64(per_solve.D, n.num_cols, "D")
        x = np.full(n.num_cols, np.nan)
        s = CSummary()
        rc = self._lib.ceres_hip_solve_unchanged_values(self._h, _p(D) if D is not None else None, per_solve.q_tolerance,
                                                        per_solve.r_tolerance, _p(x), byref(s))
        self._check_not_streaming(rc)
        summary = Summary(s.residual_norm, s.num_iterations, s.termination_type, s.message.decode(errors="replace"))
        if rc != 0:
            summary.termination_type = FATAL_ERROR
            summary.message = self._lib.ceres_hip_last_error(self._h).decode()
        return x, summary

    def solve_device(self, d_values: int, d_b: int, d_D: int, d_x: int, q_tolerance=0.0, r_tolerance=0.0):
        """Same with raw device pointers (e.g. torch tensor .data_ptr()); nothing crosses PCIe."""
        s = CSummary()
        rc = self._lib.ceres_hip_solve_device(self._h, d_values, d_b, d_D or None, q_tolerance, r_tolerance, d_x, byref(s))
        self._check_not_streaming(rc)
        summary = Summary(s.residual_norm, s.num_iterations, s.termination_type, s.message.decode(errors="replace"))
        if rc != 0:
            summary.termination_type = FATAL_ERROR
            summary.message = self._lib.ceres_hip_last_error(self._h).decode()
        return summary

    # -- f1: one trust-region step's linear algebra on the device ----------------
    def lm_compute_step(self, values, residuals, radius, eta=0.1, min_diagonal=1e-6, max_diagonal=1e32,
                        reuse_diagonal=False, values_unchanged=False, out=None):
        """LevenbergMarquardtStrategy::ComputeStep + the model-cost bookkeeping of
        TrustRegionMinimizer::ComputeTrustRegionStep.  Returns (step, Summary, model_cost_change).
        values_unchanged: the retry after a rejected step — the solver keeps the Jacobian and residuals it holds (values / residuals
        may be None): no host-to-device copy, no re-layout."""
        n = self._info
        o = CLmOptions(radius, min_diagonal, max_diagonal, eta, int(reuse_diagonal), int(values_unchanged))
        r = CLmResult()
        step = np.full(n.num_cols, np.nan) if out is None else _f64(out, n.num_cols, "out")   # out: a caller-owned (e.g. pinned) step buffer
        if values_unchanged:
            pv = pr = None
        else:
            values = _f64(values, self._values_extent, "values")
            residuals = _f64(residuals, n.num_rows, "residuals")
            pv, pr = _p(values), _p(residuals)
        self._check(self._lib.ceres_hip_lm_compute_step(self._h, pv, pr, byref(o), _p(step), byref(r)))
        s = r.linear_solver
        return step, Summary(s.residual_norm, s.num_iterations, s.termination_type, s.message.decode(errors="replace")), \
            float(r.model_cost_change)

    def lm_compute_step_device(self, d_values: int, d_residuals: int, d_step: int, radius, eta=0.1, min_diagonal=1e-6,
                               max_diagonal=1e32, reuse_diagonal=False, values_unchanged=False):
        o = CLmOptions(radius, min_diagonal, max_diagonal, eta, int(reuse_diagonal), int(values_unchanged))
        r = CLmResult()
        self._check(self._lib.ceres_hip_lm_compute_step_device(self._h, d_values, d_residuals, byref(o), d_step, byref(r)))
        s = r.linear_solver
        return Summary(s.residual_norm, s.num_iterations, s.termination_type, s.message.decode(errors="replace")), \
            float(r.model_cost_change), bool(r.step_is_finite)

    def lm_stepper(self, d_values: int, d_residuals: int, d_step: int, radius, eta=0.1, min_diagonal=1e-6, max_diagonal=1e32):
        """A callable that runs lm_compute_step_device on fixed device arrays with the argument structs built ONCE (what a C++ caller
        does: the structs live across trust-region iterations); returns the raw CLmResult, which the next call overwrites.  A timed
        loop through it pays one ctypes call per step and none of this wrapper's per-call Python work (three struct constructions,
        a message decode), during which the device idles between two steps."""
        o = CLmOptions(radius, min_diagonal, max_diagonal, eta, 0, 0)
        r = CLmResult()
        fn, h, po, pr, check = self._lib.ceres_hip_lm_compute_step_device, self._h, byref(o), byref(r), self._check
        keep = (o, r)

        def step():
            rc = fn(h, d_values, d_residuals, po, d_step, pr)
            if rc != 0:
                check(rc)
            return keep[1]
        return step

    # -- the upload hidden behind the evaluator ---------------------------------
    def values_begin(self, values, residuals):
        """values / residuals: the (pinned) host arrays the evaluator is about to fill; kept alive until values_end."""
        keep = (_f64(values, self._values_extent, "values"), _f64(residuals, self._info.num_rows, "residuals"))
        if keep[0] is not values or keep[1] is not residuals:
            raise ValueError("values_begin needs contiguous float64 arrays (they are filled in place while rows go up)")
        self._check(self._lib.ceres_hip_values_begin(self._h, _p(values), _p(residuals)))
        self._stream_keep = keep   # (only now: a refused second values_begin leaves the open session's arrays alive)

    def values_ready(self, first_row_block: int, num_row_blocks: int):
        """Thread-safe: row blocks [first, first + n) are complete."""
        rc = self._lib.ceres_hip_values_ready(self._h, int(first_row_block), int(num_row_blocks))
        if rc != 0:
            raise HipError(f"ceres_hip_values_ready: error {rc}")

    def values_end(self, column_scale=None):
        cs = _f64(column_scale, self._info.num_cols, "column_scale")
        self._check(self._lib.ceres_hip_values_end(self._h, _p(cs)))
        self._stream_keep = None

    def stream_stats(self):
        a, b, k = c_int64(0), c_int64(0), c_int32(0)
        self._check(self._lib.ceres_hip_get_stream_stats(self._h, byref(a), byref(b), byref(k)))
        return int(a.value), int(b.value), int(k.value)

    def read_loaded(self):
        """(values, residuals) as the device holds them in the handle's own copies (ceres_hip_debug_read_loaded): what a load, an LM step
        on host values or a streamed upload left in HBM, after the copy stream and the solver's stream have drained."""
        values, b = np.full(self._values_extent, np.nan), np.full(self._info.num_rows, np.nan)
        self._check(self._lib.ceres_hip_debug_read_loaded(self._h, _p(values), _p(b)))
        return values, b

    def lm_diagonal(self):
        out = np.full(self._info.num_cols, np.nan)
        self._check(self._lib.ceres_hip_get_lm_diagonal(self._h, _p(out)))
        return out

    def scale_columns(self, scale):
        scale = _f64(scale, self._info.num_cols, "scale")
        out = np.full(self._values_extent, np.nan)
        self._check(self._lib.ceres_hip_op_scale_columns(self._h, _p(scale), _p(out)))
        return out

    def set_phase_timing(self, enable: bool = True):
        """Record the per-phase HIP events of the following solves / steps (last_timing); off by default: each event record between two
        kernels idles the device for about 6 us."""
        self._check(self._lib.ceres_hip_set_phase_timing(self._h, int(bool(enable))))

    def last_timing(self) -> CTiming:
        t = CTiming()
        self._check(self._lib.ceres_hip_get_last_timing(self._h, byref(t)))
        return t

    # -- operator level ----------------------------------------------------
    def load(self, values, b=None, D=None):
        n = self._info
        self._keep = (_f64(values, self._values_extent, "values"), _f64(b, n.num_rows, "b"), _f64(D, n.num_cols, "D"))
        self._check(self._lib.ceres_hip_load(self._h, *map(_p, self._keep)))

    def load_device(self, d_values: int, d_b: int = 0, d_D: int = 0):
        self._check(self._lib.ceres_hip_load_device(self._h, d_values, d_b or None, d_D or None))

    def _xy(self, fn, x, n_out, y=None):
        x = _f64(x)
        y = np.zeros(n_out) if y is None else _f64(y).copy()
        self._check(fn(self._h, _p(x), _p(y)))
        return y

    def right_multiply(self, x, y=None):
        return self._xy(self._lib.ceres_hip_op_right_multiply, x, self._info.num_rows, y)

    def left_multiply(self, x, y=None):
        return self._xy(self._lib.ceres_hip_op_left_multiply, x, self._info.num_cols, y)

    # PartitionedMatrixView products (internal/ceres/partitioned_matrix_view_impl.h:112-375); all accumulate into y
    def right_multiply_e(self, x, y=None):
        return self._xy(self._lib.ceres_hip_op_right_multiply_e, x, self._info.num_rows, y)

    def right_multiply_f(self, x, y=None):
        return self._xy(self._lib.ceres_hip_op_right_multiply_f, x, self._info.num_rows, y)

    def left_multiply_e(self, x, y=None):
        return self._xy(self._lib.ceres_hip_op_left_multiply_e, x, self._info.num_cols_e, y)

    def left_multiply_f(self, x, y=None):
        return self._xy(self._lib.ceres_hip_op_left_multiply_f, x, self._info.num_cols_f, y)

    def _block_diagonal(self, fn, sizes):
        out = np.full(int((sizes.astype(np.int64) ** 2).sum()), np.nan)
        self._check(fn(self._h, _p(out), out.shape[0]))
        return out

    def block_diagonal_ete(self):
        return self._block_diagonal(self._lib.ceres_hip_op_block_diagonal_ete, self.bs.col_block_size[: self._info.num_e_blocks])

    def block_diagonal_ftf(self):
        return self._block_diagonal(self._lib.ceres_hip_op_block_diagonal_ftf, self.bs.col_block_size[self._info.num_e_blocks:])

    def squared_column_norm(self):
        out = np.zeros(self._info.num_cols)
        self._check(self._lib.ceres_hip_op_squared_column_norm(self._h, _p(out)))
        return out

    def jtjx(self, x):
        return self._xy(self._lib.ceres_hip_op_jtjx, x, self._info.num_cols, np.full(self._info.num_cols, np.nan))

    def jtb(self):
        out = np.full(self._info.num_cols, np.nan)
        self._check(self._lib.ceres_hip_op_jtb(self._h, _p(out)))
        return out

    def op_jacobian_gram(self, a, b):
        """ceres_hip_op_jacobian_gram: (|J a|^2, (J a).(J b), |J b|^2, (J a).f, (J b).f) on the loaded J and f, one pass over J."""
        n = self._info.num_cols
        out = np.full(5, np.nan)
        self._check(self._lib.ceres_hip_op_jacobian_gram(self._h, _p(_f64(a, n, "a")), _p(_f64(b, n, "b")), _p(out)))
        return out

    def schur_init(self):
        self._check(self._lib.ceres_hip_op_schur_init(self._h))

    def schur_rhs(self):
        out = np.full(self._info.num_cols_f, np.nan)
        self._check(self._lib.ceres_hip_get_schur_rhs(self._h, _p(out)))
        return out

    def ete_inverse(self):
        sizes = self.bs.col_block_size[: self._info.num_e_blocks].astype(np.int64)
        out = np.full(int((sizes ** 2).sum()), np.nan)
        self._check(self._lib.ceres_hip_get_ete_inverse(self._h, _p(out), out.shape[0]))
        return out

    def schur_sx(self, x):
        return self._xy(self._lib.ceres_hip_op_schur_sx, x, self._info.num_cols_f, np.full(self._info.num_cols_f, np.nan))

    def power_series_operator(self, x, y=None):
        return self._xy(self._lib.ceres_hip_op_power_series_operator, x, self._info.num_cols_f, y)

    def spse_apply(self, x, max_num_spse_iterations=5, spse_tolerance=0.0):
        x = _f64(x)
        y = np.full(self._info.num_cols_f, np.nan)
        self._check(self._lib.ceres_hip_op_spse_apply(self._h, _p(x), _p(y), max_num_spse_iterations, spse_tolerance))
        return y

    def back_substitute(self, z):
        z = _f64(z) if z is not None else np.zeros(1)
        x = np.full(self._info.num_cols, np.nan)
        self._check(self._lib.ceres_hip_op_back_substitute(self._h, _p(z), _p(x)))
        return x

    def block_jacobi_update(self):
        self._check(self._lib.ceres_hip_op_block_jacobi_update(self._h))

    def schur_jacobi_update(self):
        self._check(self._lib.ceres_hip_op_schur_jacobi_update(self._h))

    def cluster_jacobi_update(self):
        """Forms and factors the CLUSTER_JACOBI preconditioner of the loaded point; precond_apply then applies it."""
        self._check(self._lib.ceres_hip_op_cluster_jacobi_update(self._h))

    def cluster_jacobi_stats(self):
        """(number of clusters, largest cluster's scalar dimension, bytes of the factors, seconds of the host analysis)."""
        n, d, b, t = c_int32(0), c_int32(0), c_int64(0), c_double(0.0)
        self._check(self._lib.ceres_hip_cluster_jacobi_stats(self._h, byref(n), byref(d), byref(b), byref(t)))
        return n.value, d.value, b.value, t.value

    def preconditioner_blocks(self, not_inverted=False):
        i = self._info
        sizes = self.bs.col_block_size.astype(np.int64)
        if self.options.type == ITERATIVE_SCHUR:
            sizes = sizes[i.num_e_blocks:]
        out = np.full(int((sizes ** 2).sum()), np.nan)
        self._check(self._lib.ceres_hip_get_preconditioner_blocks(self._h, int(not_inverted), _p(out), out.shape[0]))
        return out

    def precond_apply(self, x, y=None):
        n = self._info.num_cols_f if self.options.type == ITERATIVE_SCHUR else self._info.num_cols
        return self._xy(self._lib.ceres_hip_op_precond_apply, x, n, y)

    def schur_eliminate_dense(self, want_rhs=True):
        n = self._info.num_cols_f
        lhs, rhs = np.full(n * n, np.nan), (np.full(n, np.nan) if want_rhs else None)
        self._check(self._lib.ceres_hip_op_schur_eliminate_dense(self._h, _p(lhs), _p(rhs)))
        return lhs.reshape(n, n), rhs

    def schur_eliminate_sparse(self):
        """(pair_i, pair_j, pair_offset, values) of the explicit Schur complement in BlockRandomAccessSparseMatrix storage."""
        npairs, nvals = c_int64(), c_int64()
        self._check(self._lib.ceres_hip_schur_storage_info(self._h, byref(npairs), byref(nvals)))
        pi, pj = np.zeros(npairs.value, np.int32), np.zeros(npairs.value, np.int32)
        off, vals = np.zeros(npairs.value, np.int64), np.full(nvals.value, np.nan)
        ip = lambda a: a.ctypes.data_as(POINTER(c_int32))
        self._check(self._lib.ceres_hip_op_schur_eliminate_sparse(self._h, ip(pi), ip(pj), off.ctypes.data_as(POINTER(c_int64)), _p(vals),
                                                                  npairs.value, nvals.value))
        return pi, pj, off, vals

    def schur_symmetric_multiply(self, x, y=None):
        return self._xy(self._lib.ceres_hip_op_schur_symmetric_multiply, x, self._info.num_cols_f, y)

    def eliminator_back_substitute(self, z):
        x = np.full(self._info.num_cols, np.nan)
        self._check(self._lib.ceres_hip_op_eliminator_back_substitute(self._h, _p(_f64(z)), _p(x)))
        return x

    def dot(self, x, y):
        x, y = _f64(x), _f64(y)
        out = np.zeros(1)
        self._check(self._lib.ceres_hip_op_dot(self._h, _p(x), _p(y), x.shape[0], _p(out)))
        return float(out[0])

    def axpby(self, a, x, b, y):
        x, y = _f64(x), _f64(y)
        z = np.zeros_like(x)
        self._check(self._lib.ceres_hip_op_axpby(self._h, a, _p(x), b, _p(y), x.shape[0], _p(z)))
        return z

    def dense_cholesky_solve(self, A: np.ndarray, b: np.ndarray, repeats: int = 1):
        """DenseCholesky::FactorAndSolve (internal/ceres/dense_cholesky.cc) on a caller-supplied SPD matrix (upper triangle
        authoritative): returns (x, average factorisation ms, failed).  What DENSE_SCHUR runs on its reduced system."""
        A = np.ascontiguousarray(A, dtype=np.float64)
        b = np.ascontiguousarray(b, dtype=np.float64)
        n = A.shape[0]
        assert A.shape == (n, n) and b.shape == (n,)
        x = np.zeros(n)
        ms, failed = c_double(0.0), c_int32(0)
        self._check(self._lib.ceres_hip_op_dense_cholesky_solve(self._h, n, _p(A), _p(b), _p(x), repeats, byref(ms), byref(failed)))
        return x, float(ms.value), bool(failed.value)

    def dense_cholesky_factor(self, A: np.ndarray, b: Optional[np.ndarray] = None, repeats: int = 1):
        """The same factorisation, debug form (ceres_hip_op_dense_cholesky_factor): the matrix and the vector lie between guard bands
        on the device.  Returns (the whole n x n array as the device left it: L in its lower triangle; x or None; failed; the number
        of guard words that changed; whether every repeat left the same bits in the lower triangle)."""
        A = np.ascontiguousarray(A, dtype=np.float64)
        n = A.shape[0]
        assert A.shape == (n, n)
        factor = np.zeros((n, n))
        x = None
        if b is not None:
            b = np.ascontiguousarray(b, dtype=np.float64)
            assert b.shape == (n,)
            x = np.zeros(n)
        failed, changed, same = c_int32(0), c_int64(-1), c_int32(0)
        self._check(self._lib.ceres_hip_op_dense_cholesky_factor(self._h, n, _p(A), _p(b) if b is not None else None, _p(factor),
                                                                 _p(x) if x is not None else None, repeats, byref(failed), byref(changed),
                                                                 byref(same)))
        return factor, x, bool(failed.value), int(changed.value), bool(same.value)

    def time_op(self, op: int, iters: int = 20) -> float:
        """Average milliseconds per application (HIP events on the solver's stream)."""
        out = np.zeros(1)
        self._check(self._lib.ceres_hip_time_op(self._h, op, iters, _p(out)))
        return float(out[0])


def comm_unique_id() -> bytes:
    buf = (c_uint8 * UNIQUE_ID_BYTES)()
    rc = load_library().ceres_hip_comm_get_unique_id(buf)
    if rc != 0:
        raise HipError(f"ncclGetUniqueId failed ({rc})")
    return bytes(buf)


def create_linear_solver(options: LinearSolverOptions, bs: BlockStructure, **kw) -> HipLinearSolver:
    """LinearSolver::Create with the reference's fall-backs (internal/ceres/linear_solver.cc:51-73,
    internal/ceres/preconditioner.cc:39-47): ITERATIVE_SCHUR without eliminated blocks becomes CGNR,
    and SCHUR_JACOBI becomes JACOBI with it."""
    import copy
    o = copy.copy(options)
    nelim = o.elimination_groups[0] if o.elimination_groups else 0
    if o.type == ITERATIVE_SCHUR and nelim == 0:
        o.type = CGNR
        if o.preconditioner_type == SCHUR_JACOBI:
            o.preconditioner_type = JACOBI
    s = HipLinearSolver(o, **kw)
    s.set_structure(bs)
    return s


def debug_plan(bs: BlockStructure, num_eliminate_blocks: int):
    """The host-side tile packing plan (no device needed).  Returns a dict or {'eligible': False, 'why': ...}."""
    lib = load_library()
    c = bs.as_ctypes()
    eligible, n_tiles = c_int32(), c_int64()
    why = ctypes.create_string_buffer(256)
    null32, nullu = POINTER(c_int32)(), POINTER(c_uint32)()
    rc = lib.ceres_hip_debug_plan(byref(c), num_eliminate_blocks, byref(eligible), byref(n_tiles), null32, null32, null32,
                                  nullu, null32, null32, 0, why, 256)
    if rc != 0 or not eligible.value:
        return {"eligible": False, "why": why.value.decode()}
    nt = n_tiles.value
    ns = nt * 64
    row, cam, pt = (np.zeros(ns, np.int32) for _ in range(3))
    seg = np.zeros(ns, np.uint32)
    kind, aux = np.zeros(nt, np.int32), np.zeros(nt, np.int32)
    ip = lambda a: a.ctypes.data_as(POINTER(c_int32))
    rc = lib.ceres_hip_debug_plan(byref(c), num_eliminate_blocks, byref(eligible), byref(n_tiles), ip(row), ip(cam), ip(pt),
                                  seg.ctypes.data_as(POINTER(c_uint32)), ip(kind), ip(aux), ns, why, 256)
    assert rc == 0
    return {"eligible": True, "n_tiles": nt, "slot_row": row, "slot_cam": cam, "slot_pt": pt, "seg_first": seg & 0xff,
            "seg_last": (seg >> 8) & 0xff, "valid": (seg >> 16) & 1, "tail_a": (seg >> 17) & 63, "has_a": (seg >> 23) & 1,
            "tail_b": (seg >> 24) & 63, "has_b": (seg >> 30) & 1, "tile_kind": kind, "tile_aux": aux}


def debug_value_streams(bs: BlockStructure):
    """The plan of the streamed upload (csrc/plan.cc, PlanValueStreams; no device): (streams, lo, hi) with lo / hi of shape
    (2, num_row_blocks) — row blocks [r0, r1) own the doubles [lo[k, r0], hi[k, r1 - 1]) of the value array in class k < streams."""
    lib = load_library()
    c = bs.as_ctypes()
    k = c_int32(-1)
    lo, hi = (np.zeros((2, int(bs.num_row_blocks)), dtype=np.int64) for _ in range(2))
    rc = lib.ceres_hip_debug_value_streams(byref(c), byref(k), lo.ctypes.data_as(POINTER(c_int64)), hi.ctypes.data_as(POINTER(c_int64)))
    if rc != 0:
        raise HipError(f"ceres_hip_debug_value_streams: error {rc}")
    return int(k.value), lo, hi


def debug_cluster_cameras(bs: BlockStructure, num_eliminate_blocks: int, visibility_clustering_type: int = CANONICAL_VIEWS):
    """ceres_hip_debug_cluster_cameras: (cluster of every F block, number of clusters) — the host analysis of CLUSTER_JACOBI, no device."""
    lib = load_library()
    c = bs.as_ctypes()
    nf = int(bs.num_col_blocks) - int(num_eliminate_blocks)
    membership = np.full(max(nf, 1), -1, dtype=np.int32)
    n = c_int32(0)
    rc = lib.ceres_hip_debug_cluster_cameras(byref(c), int(num_eliminate_blocks), int(visibility_clustering_type),
                                             membership.ctypes.data_as(POINTER(c_int32)), byref(n))
    if rc != 0:
        raise HipError(f"ceres_hip_debug_cluster_cameras: error {rc}")
    return membership[:max(nf, 0)], n.value


def debug_staged_x_plan(bs: BlockStructure, num_eliminate_blocks: int):
    """Which cameras' part of x the streaming kernels keep in LDS beside the accumulators (csrc/plan.cc, BalPlan::xhot_cam; no device
    needed).  Returns None for structures off the fused path."""
    lib = load_library()
    c = bs.as_ctypes()
    counts = (c_int64 * 4)()
    n32 = POINTER(c_int32)()
    fn = lib.ceres_hip_debug_staged_x_plan
    if fn(byref(c), c_int32(num_eliminate_blocks), counts, n32, n32, c_int64(0), c_int64(0)) != 0:
        return None
    nt, ncam, nst, acc_bytes = (int(v) for v in counts)
    staged, word = np.zeros(max(nst, 1), np.int32), np.zeros(nt * 64, np.int32)
    ip = lambda a: a.ctypes.data_as(POINTER(c_int32))
    assert fn(byref(c), c_int32(num_eliminate_blocks), counts, ip(staged), ip(word), c_int64(nst), c_int64(nt * 64)) == 0
    return {"n_tiles": nt, "n_cameras": ncam, "staged_cam": staged[:nst], "accumulator_bytes": acc_bytes, "slot_word": word}


def debug_hybrid_plan(bs: BlockStructure, num_eliminate_blocks: int, groups: int, rows: int):
    """The camera-accumulation plan for more cameras than LDS rows (csrc/plan.cc; no device needed): hybrid for groups >= 2,
    spill-everything for groups = 0.  Returns None when the structure is not <2,3,9>-shaped or its cameras fit in LDS."""
    lib = load_library()
    c = bs.as_ctypes()
    counts = (c_int64 * 8)()
    n32 = POINTER(c_int32)()
    fn = lib.ceres_hip_debug_hybrid_plan
    rc = fn(byref(c), c_int32(num_eliminate_blocks), c_int32(groups), c_int32(rows), counts, n32, n32, n32, n32, n32, n32, n32, n32,
            c_int64(0), c_int64(0), c_int64(0))
    if rc != 0:
        return None
    nt, hyb, k, kh, flush0, ring_rows, ne, nu = (int(v) for v in counts)
    word, row = np.zeros(nt * 64, np.int32), np.zeros(nt * 64, np.int32)
    zbase, grp = np.zeros(nt, np.int32), np.zeros(max(groups, 0) + 1, np.int32)
    ent, ucam, ub, ue = np.zeros(ne, np.int32), np.zeros(nu, np.int32), np.zeros(nu, np.int32), np.zeros(nu, np.int32)
    ip = lambda a: a.ctypes.data_as(POINTER(c_int32))
    rc = fn(byref(c), c_int32(num_eliminate_blocks), c_int32(groups), c_int32(rows), counts, ip(word), ip(row), ip(zbase), ip(grp), ip(ent),
            ip(ucam), ip(ub), ip(ue), c_int64(nt * 64), c_int64(ne), c_int64(nu))
    assert rc == 0
    valid = word != -1   # (a spilled slot's word has its top bits set: negative as int32, but never -1)
    uw = word.view(np.uint32)
    return {"n_tiles": nt, "hybrid": bool(hyb), "rows": k, "hot_rows": kh, "flush_row0": flush0, "ring_rows": ring_rows,
            "valid": valid, "slot_cam": np.where(valid, (uw & 0xFFFFF).astype(np.int64), -1),
            "slot_acc": np.where(valid, (uw >> 20).astype(np.int64), 0xFFF),
            "slot_row": row, "tile_zbase": zbase, "grp_tile_ptr": grp if hyb else None, "entry_row": ent, "unit_cam": ucam,
            "unit_begin": ub, "unit_end": ue}


def debug_long_rounds(bs: BlockStructure, num_eliminate_blocks: int, renumber: bool = True, groups: int = 0, rows: int = 0):
    """Where the plan puts the points of more than 64 observations and the rounds the streaming kernels take them in
    (csrc/plan.cc; no device needed).  Returns None when the structure is not <2,3,9>-shaped."""
    lib = load_library()
    c = bs.as_ctypes()
    counts = (c_int64 * 5)()
    n32, nu = POINTER(c_int32)(), POINTER(c_uint32)()
    fn = lib.ceres_hip_debug_long_rounds
    args = (byref(c), c_int32(num_eliminate_blocks), c_int32(1 if renumber else 0), c_int32(groups), c_int32(rows), counts)
    if fn(*args, n32, n32, n32, n32, n32, n32, n32, nu, c_int64(0), c_int64(0), c_int64(0)) != 0:
        return None
    nt, nr, nrounds, behind, nseq = (int(v) for v in counts)
    kind, aux = np.zeros(nt, np.int32), np.zeros(nt, np.int32)
    rtp, lp, rp = np.zeros(nr + 1, np.int32), np.zeros(nr, np.int32), np.zeros(nr + 1, np.int32)
    sp, flag = np.zeros(nrounds + 1, np.int32), np.zeros(max(nrounds, 1), np.int32)
    words = np.zeros(max(nrounds, 1) * 8, np.uint32)
    ip = lambda a: a.ctypes.data_as(POINTER(c_int32))
    rc = fn(*args, ip(kind), ip(aux), ip(rtp), ip(lp), ip(rp), ip(sp), ip(flag), words.ctypes.data_as(POINTER(c_uint32)), c_int64(nt),
            c_int64(nr), c_int64(nrounds))
    assert rc == 0
    return {"n_tiles": nt, "tile_kind": kind, "tile_aux": aux, "range_tile_ptr": rtp, "long_ptr": lp, "round_ptr": rp,
            "seq_ptr": sp[:nseq + 1], "round_flag": flag[:nrounds], "round_word": words[:nrounds * 8].reshape(nrounds, 8),
            "long_behind": bool(behind)}


CONVERGENCE, MINIMIZER_NO_CONVERGENCE, MINIMIZER_FAILURE = 0, 1, 2
# CERES_HIP_LOSS_* (include/ceres_hip.h): the robust losses of BalProblem.set_loss, by name
LOSS_TRIVIAL, LOSS_HUBER, LOSS_SOFTLONE, LOSS_CAUCHY, LOSS_ARCTAN, LOSS_TOLERANT, LOSS_TUKEY = range(7)
LOSSES = {"trivial": LOSS_TRIVIAL, "huber": LOSS_HUBER, "soft_l_one": LOSS_SOFTLONE, "cauchy": LOSS_CAUCHY, "arctan": LOSS_ARCTAN,
          "tolerant": LOSS_TOLERANT, "tukey": LOSS_TUKEY}
# CERES_HIP_INNER_* (include/ceres_hip.h): the orderings of BalProblem.set_inner_iterations, by bundle_adjuster's
# --blocks_for_inner_iterations name
INNER_NONE, INNER_AUTOMATIC, INNER_CAMERAS, INNER_POINTS, INNER_CAMERAS_POINTS, INNER_POINTS_CAMERAS = range(6)
INNER_BLOCKS = {None: INNER_NONE, "automatic": INNER_AUTOMATIC, "cameras": INNER_CAMERAS, "points": INNER_POINTS,
                "cameras,points": INNER_CAMERAS_POINTS, "points,cameras": INNER_POINTS_CAMERAS}


# CERES_HIP_LEVENBERG_MARQUARDT / CERES_HIP_DOGLEG and CERES_HIP_{TRADITIONAL,SUBSPACE}_DOGLEG (include/ceres_hip.h), by bundle_adjuster's
# --trust_region_strategy / --dogleg names (without the _dogleg suffix)
LEVENBERG_MARQUARDT, DOGLEG = 0, 1
TRADITIONAL_DOGLEG, SUBSPACE_DOGLEG = 0, 1
TRUST_REGION_STRATEGIES = {"levenberg_marquardt": LEVENBERG_MARQUARDT, "dogleg": DOGLEG}
DOGLEG_TYPES = {"traditional": TRADITIONAL_DOGLEG, "subspace": SUBSPACE_DOGLEG}
# what ceres_hip_debug_dogleg_subspace_minimum returns besides 0: the cases that fall back to the traditional step
DOGLEG_NO_ROOT, DOGLEG_COSINE = 1, 2


# CERES_HIP_CAMERA_* (include/ceres_hip.h): the camera models of BalProblem, by name — bundle_adjuster's default, --use_quaternions, and
# --use_quaternions --use_manifolds
CAMERA_ANGLE_AXIS, CAMERA_QUATERNION, CAMERA_QUATERNION_MANIFOLD = 0, 1, 2
CAMERA_MODELS = {"angle_axis": CAMERA_ANGLE_AXIS, "quaternion": CAMERA_QUATERNION, "quaternion_manifold": CAMERA_QUATERNION_MANIFOLD}


def angle_axis_to_quaternion(a):
    """AngleAxisToQuaternion (include/ceres/rotation.h), row-wise on an (n, 3) array: (n, 4) [w x y z]."""
    a = np.asarray(a, dtype=np.float64).reshape(-1, 3)
    theta = np.sqrt(np.sum(a * a, axis=1))
    nz = theta != 0.0
    th = np.where(nz, theta, 1.0)
    k = np.where(nz, np.sin(0.5 * th) / th, 0.5)
    return np.concatenate([np.where(nz, np.cos(0.5 * th), 1.0)[:, None], a * k[:, None]], axis=1)


def quaternion_to_angle_axis(q):
    """QuaternionToAngleAxis (include/ceres/rotation.h), row-wise on an (n, 4) [w x y z] array: (n, 3), angle in [-pi, pi]."""
    q = np.asarray(q, dtype=np.float64).reshape(-1, 4)
    v = q[:, 1:]
    sin_theta = np.sqrt(np.sum(v * v, axis=1))
    nz = sin_theta != 0.0
    sign = np.copysign(1.0, q[:, 0])
    st = np.where(nz, sin_theta, 1.0)
    k = np.where(nz, 2.0 * np.arctan2(sign * sin_theta, sign * q[:, 0]) / st, 2.0)
    return v * k[:, None]


def dogleg_subspace_minimum(B, g, radius):
    """ceres_hip_debug_dogleg_subspace_minimum: (code, x) — the unscaled boundary minimiser x of 1/2 x'Bx + g'x for the 2x2 B, and 0,
    DOGLEG_NO_ROOT or DOGLEG_COSINE."""
    lib = load_library()
    Bm = np.ascontiguousarray(B, dtype=np.float64).reshape(4)
    gv = np.ascontiguousarray(g, dtype=np.float64).reshape(2)
    x = np.zeros(2)
    rc = lib.ceres_hip_debug_dogleg_subspace_minimum(_p(Bm), _p(gv), float(radius), _p(x))
    if rc < 0:
        raise HipError(f"ceres_hip_debug_dogleg_subspace_minimum: error {rc}")
    return rc, x


def line_search_options(**opts) -> CLineSearchOptions:
    """ceres_hip_line_search_default_options with the given fields replaced."""
    o = CLineSearchOptions()
    load_library().ceres_hip_line_search_default_options(byref(o))
    for k, val in opts.items():
        if not hasattr(o, k):
            raise TypeError(f"unknown line search option {k}")
        setattr(o, k, val)
    return o


def debug_line_search(fn, step_size_estimate, initial_cost, initial_gradient, **opts) -> CLineSearchResult:
    """ceres_hip_debug_line_search: one LineSearch::Search on fn(x, want_gradient) -> (value, gradient) or None (an invalid sample)."""
    lib = load_library()
    o = line_search_options(**opts)

    def trampoline(x, want_gradient, value, gradient, user):
        r = fn(x, bool(want_gradient))
        if r is None:
            return 1
        value[0] = r[0]
        gradient[0] = r[1]
        return 0
    out = CLineSearchResult()
    cb = UNIVARIATE_FN(trampoline)   # (kept alive until the call returns)
    rc = lib.ceres_hip_debug_line_search(byref(o), ctypes.cast(cb, c_void_p), None, float(step_size_estimate), float(initial_cost),
                                         float(initial_gradient), byref(out))
    if rc != 0:
        raise HipError(f"ceres_hip_debug_line_search: error {rc}: {lib.ceres_hip_bal_last_error(None).decode()}")
    return out


def debug_minimize_interpolating_polynomial(x, value, value_valid, gradient, gradient_valid, x_min, x_max):
    """ceres_hip_debug_minimize_interpolating_polynomial: (optimal_x, optimal_value, coefficients — highest power first)."""
    lib = load_library()
    xs = np.ascontiguousarray(x, dtype=np.float64)
    v = np.ascontiguousarray(value, dtype=np.float64)
    g = np.ascontiguousarray(gradient, dtype=np.float64)
    vv = np.ascontiguousarray(value_valid, dtype=np.int32)
    gv = np.ascontiguousarray(gradient_valid, dtype=np.int32)
    ox, ov, coef = np.zeros(1), np.zeros(1), np.zeros(6)
    rc = lib.ceres_hip_debug_minimize_interpolating_polynomial(xs.shape[0], _p(xs), _p(v), vv.ctypes.data_as(POINTER(c_int32)), _p(g),
                                                               gv.ctypes.data_as(POINTER(c_int32)), float(x_min), float(x_max), _p(ox),
                                                               _p(ov), _p(coef))
    if rc != 0:
        raise HipError(f"ceres_hip_debug_minimize_interpolating_polynomial: error {rc}: {lib.ceres_hip_bal_last_error(None).decode()}")
    return float(ox[0]), float(ov[0]), coef[:int(vv.astype(bool).sum() + gv.astype(bool).sum())].copy()


def debug_lbfgs_direction(rank, delta_x, delta_gradient, gradient, use_scaling=False):
    """ceres_hip_debug_lbfgs_direction (device 0): (-H gradient, accepted flag per update) for the updates fed in order."""
    lib = load_library()
    g = np.ascontiguousarray(gradient, dtype=np.float64)
    n = g.shape[0]
    dx = np.ascontiguousarray(delta_x, dtype=np.float64).reshape(-1, n)
    dg = np.ascontiguousarray(delta_gradient, dtype=np.float64).reshape(-1, n)
    d = np.empty(n)
    acc = np.zeros(max(dx.shape[0], 1), dtype=np.int32)
    rc = lib.ceres_hip_debug_lbfgs_direction(n, int(rank), int(bool(use_scaling)), dx.shape[0], _p(dx), _p(dg), _p(g), _p(d),
                                             acc.ctypes.data_as(POINTER(c_int32)))
    if rc != 0:
        raise HipError(f"ceres_hip_debug_lbfgs_direction: error {rc}: {lib.ceres_hip_bal_last_error(None).decode()}")
    return d, acc[:dx.shape[0]].copy()


def inner_iteration_ordering(num_cameras, num_points, camera_index, point_index, blocks="automatic"):
    """ceres_hip_debug_inner_iteration_ordering: (group of every block in state order — points, then cameras; -1 outside —, groups)."""
    lib = load_library()
    cam = np.ascontiguousarray(camera_index, dtype=np.int32)
    pt = np.ascontiguousarray(point_index, dtype=np.int32)
    kind = INNER_BLOCKS[blocks] if blocks is None or isinstance(blocks, str) else int(blocks)
    out = np.empty(int(num_points) + int(num_cameras), dtype=np.int32)
    ng = c_int32()
    rc = lib.ceres_hip_debug_inner_iteration_ordering(int(num_cameras), int(num_points), cam.shape[0], cam.ctypes.data_as(POINTER(c_int32)),
                                                      pt.ctypes.data_as(POINTER(c_int32)), kind, out.ctypes.data_as(POINTER(c_int32)), byref(ng))
    if rc != 0:
        raise HipError(f"ceres_hip_debug_inner_iteration_ordering: error {rc}")
    return out, ng.value


def _constant_mask(which, n, name):
    """None / an empty sequence -> None; a boolean mask of length n or an array of block indices -> a uint8 mask."""
    if which is None:
        return None
    a = np.asarray(which)
    if a.size == 0:
        return None
    if a.dtype == np.bool_:
        if a.shape != (n,):
            raise ValueError(f"{name}: a boolean mask must have {n} entries")
        return np.ascontiguousarray(a, dtype=np.uint8)
    idx = a.astype(np.int64).reshape(-1)
    if idx.min() < 0 or idx.max() >= n:
        raise ValueError(f"{name}: block index out of range")
    m = np.zeros(n, dtype=np.uint8)
    m[idx] = 1
    return m


def _u8p(a):
    return a.ctypes.data_as(POINTER(ctypes.c_uint8)) if a is not None else None


def debug_bal_reduce(num_cameras, num_points, camera_index, point_index, constant_cameras=None, constant_points=None):
    """ceres_hip_debug_bal_reduce (host code, no device): what ceres_hip_bal_create_with_constant_blocks makes of the problem.
    Returns (row_observation[num_rows], num_rows_e, camera_column, point_column); HipError with the library's message when refused."""
    lib = load_library()
    cam = np.ascontiguousarray(camera_index, dtype=np.int32) if camera_index is not None else None
    pt = np.ascontiguousarray(point_index, dtype=np.int32) if point_index is not None else None
    no = int(cam.shape[0]) if cam is not None else (int(pt.shape[0]) if pt is not None else 0)
    cm = _constant_mask(constant_cameras, int(num_cameras), "constant_cameras")
    pm = _constant_mask(constant_points, int(num_points), "constant_points")
    rows = np.empty(max(no, 1), dtype=np.int32)
    ccol = np.empty(max(int(num_cameras), 1), dtype=np.int32)
    pcol = np.empty(max(int(num_points), 1), dtype=np.int32)
    nr, ne = c_int64(), c_int64()
    i32 = lambda a: a.ctypes.data_as(POINTER(c_int32)) if a is not None else None
    rc = lib.ceres_hip_debug_bal_reduce(int(num_cameras), int(num_points), no, i32(cam), i32(pt), _u8p(cm), _u8p(pm), byref(nr), byref(ne),
                                        i32(rows), i32(ccol), i32(pcol))
    if rc != 0:
        raise HipError(f"ceres_hip error {rc}: {lib.ceres_hip_bal_last_error(None).decode()}")
    return rows[:nr.value].copy(), ne.value, ccol[:int(num_cameras)], pcol[:int(num_points)]


INTRINSIC_NAMES = ("f", "k1", "k2")   # coordinates 6, 7, 8 of the angle-axis camera [angle-axis(3) t(3) f k1 k2]


def _intrinsics_mask(spec, camera_state_size):
    """constant_intrinsics -> a uint8 mask of camera_state_size entries, or None for nothing marked.  spec: names from INTRINSIC_NAMES,
    coordinate indices, or a boolean mask of camera_state_size entries.  What may be marked is the library's rule (its message)."""
    if spec is None:
        return None
    if isinstance(spec, str):
        spec = [spec]
    items = list(spec)
    if len(items) == 0:
        return None
    m = np.zeros(camera_state_size, dtype=np.uint8)
    if all(isinstance(v, (bool, np.bool_)) for v in items):
        if len(items) != camera_state_size:
            raise ValueError(f"constant_intrinsics: a boolean mask has {camera_state_size} entries, got {len(items)}")
        m[:] = np.asarray(items, dtype=bool)
    else:
        for v in items:
            if isinstance(v, str):
                if v not in INTRINSIC_NAMES:
                    raise ValueError(f"constant_intrinsics: unknown name {v!r}: one of {', '.join(INTRINSIC_NAMES)}")
                m[6 + INTRINSIC_NAMES.index(v)] = 1
            else:
                j = int(v)
                if j < 0 or j >= camera_state_size:
                    raise ValueError(f"constant_intrinsics: coordinate {j} outside [0, {camera_state_size})")
                m[j] = 1
    return m if m.any() else None


class BalProblem:
    """Bundle adjustment in BAL form on the device: the Evaluator of the reduced,
    Schur-ordered program (internal/ceres/evaluator.h:98-158) for the Snavely reprojection error
    (examples/snavely_reprojection_error.h:53-105, examples/bal_problem.cc:75-135) and
    TrustRegionMinimizer::Minimize around the linear solver `options` selects.

    state = [3 doubles per point | 9 doubles per camera]; `state_from_bal` / `state_to_bal`
    convert from the file order (cameras, then points).

    camera_model = "angle_axis" (the default), "quaternion" (bundle_adjuster --use_quaternions: cameras [q_w q_x q_y q_z | t | f k1 k2],
    Euclidean Plus) or "quaternion_manifold" (--use_quaternions --use_manifolds: QuaternionManifold on q) — or a CAMERA_* number.  The
    state is ambient (num_parameters: 10 per quaternion camera); gradients are tangent (num_effective_parameters: 9 per camera with
    the manifold).

    constant_cameras / constant_points (Problem::SetParameterBlockConstant): index arrays or boolean masks of the blocks to hold fixed;
    None or empty takes the entry points above.  The state keeps its full layout (constant blocks are read, never written); the
    gradient, the Jacobian's columns and minimize's step are the reduced program's — free points, then free cameras, ascending — see
    ceres_hip_bal_create_with_constant_blocks in include/ceres_hip.h, `reduced_sizes` and `fixed_cost`.

    constant_intrinsics (SubsetManifold on every camera block): names from ("f", "k1", "k2"), coordinate indices 6 .. 8 or a boolean
    mask of nine — the intrinsics held fixed on all cameras while poses and points move; angle-axis cameras only.  The state stays
    nine per camera (marked coordinates are read, never written); `camera_tangent_size` = 9 - (number marked) is the width of a
    camera in the gradient, the step and the Jacobian — see ceres_hip_bal_create_with_fixed_intrinsics in include/ceres_hip.h for what
    such a handle offers.

    camera_groups (shared intrinsics: one [f, k1, k2] parameter block per group of cameras beside a 6-wide pose block per camera, as
    examples/libmv_bundle_adjuster.cc builds its problem): a sequence of num_cameras ints in [0, num_groups), every id used; angle-axis
    cameras only, exclusive with constant_intrinsics and constant_points.  The state stays nine per camera, the intrinsics of a group
    bit-identical in all its cameras; the gradient and the step are [points | free cameras' poses | groups]
    (`num_effective_parameters`), `camera_tangent_size` is 6 and `num_intrinsics_groups` the number of groups; constant_cameras holds
    poses constant — see ceres_hip_bal_create_with_shared_intrinsics in include/ceres_hip.h for what such a handle offers."""

    def __init__(self, options: LinearSolverOptions, num_cameras, num_points, camera_index, point_index, observations,
                 camera_model="angle_axis", constant_cameras=None, constant_points=None, constant_intrinsics=None, camera_groups=None):
        self._lib = load_library()
        self.options = options
        if isinstance(camera_model, str):
            if camera_model not in CAMERA_MODELS:
                raise ValueError(f"unknown camera model {camera_model!r}: one of {', '.join(CAMERA_MODELS)}")
            camera_model = CAMERA_MODELS[camera_model]
        self.camera_model = int(camera_model)
        self.num_cameras, self.num_points = int(num_cameras), int(num_points)
        cam = np.ascontiguousarray(camera_index, dtype=np.int32)
        pt = np.ascontiguousarray(point_index, dtype=np.int32)
        obs = _f64(observations).reshape(-1)
        self.num_observations = int(cam.shape[0])
        if pt.shape[0] != self.num_observations or obs.shape[0] != 2 * self.num_observations:
            raise ValueError("camera_index, point_index and observations disagree on the number of observations")
        c = COptions(options.type, options.preconditioner_type, options.min_num_iterations,
                     options.max_num_iterations, options.residual_reset_period, self.num_points, options.device,
                     int(options.force_generic_path), options.cg_check_interval, options.jacobian_storage,
                     options.max_num_spse_iterations, int(options.use_spse_initialization), options.spse_tolerance,
                     int(options.use_explicit_schur_complement), int(options.visibility_clustering_type))
        cm = _constant_mask(constant_cameras, self.num_cameras, "constant_cameras")
        pm = _constant_mask(constant_points, self.num_points, "constant_points")
        im = _intrinsics_mask(constant_intrinsics, 9 if self.camera_model == CAMERA_ANGLE_AXIS else 10)
        self.num_intrinsics_groups = 0
        if camera_groups is not None:
            if im is not None or pm is not None:
                raise ValueError("camera_groups cannot be combined with constant_intrinsics or constant_points")
            groups = np.ascontiguousarray(camera_groups, dtype=np.int32).reshape(-1)
            if groups.shape[0] != self.num_cameras:
                raise ValueError(f"camera_groups has one entry per camera: {self.num_cameras}, got {groups.shape[0]}")
            # (the number of groups is the largest id + 1: an unused or negative id, or a quaternion model, is the library's refusal)
            ng = int(groups.max()) + 1
            self._h = self._lib.ceres_hip_bal_create_with_shared_intrinsics(byref(c), self.camera_model, self.num_cameras, self.num_points,
                                                                            self.num_observations, cam.ctypes.data_as(POINTER(c_int32)),
                                                                            pt.ctypes.data_as(POINTER(c_int32)), _p(obs), _u8p(cm),
                                                                            groups.ctypes.data_as(POINTER(c_int32)), ng)
            self.num_intrinsics_groups = ng
        elif im is not None:
            self._h = self._lib.ceres_hip_bal_create_with_fixed_intrinsics(byref(c), self.camera_model, self.num_cameras, self.num_points,
                                                                           self.num_observations, cam.ctypes.data_as(POINTER(c_int32)),
                                                                           pt.ctypes.data_as(POINTER(c_int32)), _p(obs), _u8p(cm), _u8p(pm),
                                                                           _u8p(im))
        elif cm is not None or pm is not None:
            self._h = self._lib.ceres_hip_bal_create_with_constant_blocks(byref(c), self.camera_model, self.num_cameras, self.num_points,
                                                                          self.num_observations, cam.ctypes.data_as(POINTER(c_int32)),
                                                                          pt.ctypes.data_as(POINTER(c_int32)), _p(obs), _u8p(cm), _u8p(pm))
        elif self.camera_model == CAMERA_ANGLE_AXIS:
            self._h = self._lib.ceres_hip_bal_create(byref(c), self.num_cameras, self.num_points, self.num_observations,
                                                     cam.ctypes.data_as(POINTER(c_int32)), pt.ctypes.data_as(POINTER(c_int32)),
                                                     _p(obs))
        else:
            self._h = self._lib.ceres_hip_bal_create_with_camera(byref(c), self.camera_model, self.num_cameras, self.num_points,
                                                                 self.num_observations, cam.ctypes.data_as(POINTER(c_int32)),
                                                                 pt.ctypes.data_as(POINTER(c_int32)), _p(obs))
        if not self._h:
            raise HipError(self._lib.ceres_hip_bal_last_error(None).decode())
        n, m, v, t = c_int64(), c_int64(), c_int64(), c_int64()
        self._check(self._lib.ceres_hip_bal_sizes(self._h, byref(n), byref(m), byref(v)))
        self._check(self._lib.ceres_hip_bal_num_effective_parameters(self._h, byref(t)))
        self.num_parameters, self.num_residuals, self.num_jacobian_values = n.value, m.value, v.value
        self.num_effective_parameters = t.value
        self.camera_state_size = 9 if self.camera_model == CAMERA_ANGLE_AXIS else 10
        # Jacobian columns per camera: the tangent of the manifold, less the coordinates constant_intrinsics marks
        self.camera_tangent_size = (10 if self.camera_model == CAMERA_QUATERNION else 9) - (int(im.sum()) if im is not None else 0)
        if self.num_intrinsics_groups:   # (the pose; the intrinsics are the groups' blocks)
            self.camera_tangent_size = 6
        self.num_rows = self.num_residuals // 2   # (= num_observations without constant blocks)

    @classmethod
    def from_file(cls, options: LinearSolverOptions, filename, camera_model="angle_axis"):
        """BALProblem(filename, use_quaternions) (examples/bal_problem.cc:75-135).  Returns (problem, initial state)."""
        from . import problems
        nc, npts, cam, pt, obs, par = problems.read_bal(filename)
        p = cls(options, nc, npts, cam, pt, obs, camera_model=camera_model)
        return p, p.state_from_bal(par)

    def _check(self, rc):
        if rc != 0:
            raise HipError(f"ceres_hip error {rc}: {self._lib.ceres_hip_bal_last_error(self._h).decode()}")

    def close(self):
        if getattr(self, "_h", None):
            self._lib.ceres_hip_bal_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def solver_info(self) -> CInfo:
        """ceres_hip_get_info of the linear solver inside (which kernels its structure runs on, the tile plan)."""
        i = CInfo()
        self._check(self._lib.ceres_hip_get_info(self._lib.ceres_hip_bal_linear_solver(self._h), byref(i)))
        return i

    def preconditioner_blocks(self, not_inverted=False):
        """The block-diagonal preconditioner of the LAST linear solve inside minimize (camera blocks; CGNR: point blocks first)."""
        _, _, _, nfc, nfp = self.reduced_sizes()
        w = self.num_effective_parameters - 3 * nfp
        w //= max(1, nfc)
        n = w * w * nfc + (9 * nfp if self.options.type == CGNR else 0)
        out = np.full(n, np.nan)
        inner = self._lib.ceres_hip_bal_linear_solver(self._h)
        rc = self._lib.ceres_hip_get_preconditioner_blocks(inner, int(not_inverted), _p(out), n)
        if rc != 0:
            raise HipError(f"ceres_hip error {rc}: {self._lib.ceres_hip_last_error(inner).decode()}")
        return out

    def evaluate_tiles_timing(self, state, flags=0, iters=20) -> float:
        """Average microseconds of the tile-order evaluator's launch (experiments: flags switch groups of its stores off)."""
        x = _f64(state, self.num_parameters)
        out = np.zeros(1)
        self._check(self._lib.ceres_hip_debug_bal_evaluate_tiles_timing(self._h, _p(x), int(flags), int(iters), _p(out)))
        return float(out[0])

    def reduced_sizes(self):
        """(rows kept, rows with an E cell — they come first —, rows removed because both blocks are constant, free cameras, free points)."""
        a, b, c = c_int64(), c_int64(), c_int64()
        d, e = c_int32(), c_int32()
        self._check(self._lib.ceres_hip_bal_reduced_sizes(self._h, byref(a), byref(b), byref(c), byref(d), byref(e)))
        return a.value, b.value, c.value, d.value, e.value

    def fixed_cost(self, state):
        """Solver::Summary::fixed_cost at state: the removed rows' cost with the loss in force (minimize's costs include it)."""
        x = _f64(state, self.num_parameters)
        out = np.zeros(1)
        self._check(self._lib.ceres_hip_bal_fixed_cost(self._h, _p(x), _p(out)))
        return float(out[0])

    def row_order(self):
        out = np.empty(self.num_rows, dtype=np.int32)
        self._check(self._lib.ceres_hip_bal_get_row_order(self._h, out.ctypes.data_as(POINTER(c_int32))))
        return out

    def state_from_bal(self, parameters):
        """BAL file order (9 per camera, then 3 per point) -> state; quaternion cameras through AngleAxisToQuaternion, as
        BALProblem(filename, use_quaternions = true) converts them (examples/bal_problem.cc:110-131)."""
        a = _f64(parameters, 9 * self.num_cameras + 3 * self.num_points)
        cams = a[:9 * self.num_cameras]
        if self.camera_model != CAMERA_ANGLE_AXIS:
            c9 = cams.reshape(-1, 9)
            cams = np.concatenate([angle_axis_to_quaternion(c9[:, :3]), c9[:, 3:]], axis=1).reshape(-1)
        return np.concatenate([a[9 * self.num_cameras:9 * self.num_cameras + 3 * self.num_points], cams])

    def state_to_bal(self, state):
        """state -> BAL file order; quaternion cameras through QuaternionToAngleAxis (BALProblem::WriteToFile, examples/bal_problem.cc:157-160)."""
        a = _f64(state, self.num_parameters)
        cams = a[3 * self.num_points:]
        if self.camera_model != CAMERA_ANGLE_AXIS:
            c10 = cams.reshape(-1, 10)
            cams = np.concatenate([quaternion_to_angle_axis(c10[:, :4]), c10[:, 4:]], axis=1).reshape(-1)
        return np.concatenate([cams, a[:3 * self.num_points]])

    def set_loss(self, kind, a=1.0, b=1.0, scale=1.0):
        """The robust loss of every observation, ScaledLoss(kind(a[, b]), scale) (include/ceres/loss_function.h): "trivial", "huber",
        "soft_l_one", "cauchy", "arctan", "tolerant" (a and b) or "tukey" — or a LOSS_* number.  bundle_adjuster --robustify is
        set_loss("huber", 1.0).  In force for later evaluate / minimize calls until set again; "trivial" with scale 1 is the squared loss."""
        if isinstance(kind, str):
            if kind not in LOSSES:
                raise ValueError(f"unknown loss kind {kind!r}: one of {', '.join(LOSSES)}")
            kind = LOSSES[kind]
        self._check(self._lib.ceres_hip_bal_set_loss(self._h, int(kind), float(a), float(b), float(scale)))

    def set_inner_iterations(self, blocks="automatic", tolerance=1e-3):
        """Inner iterations after every trust-region step of minimize (Solver::Options::use_inner_iterations, inner_iteration_ordering,
        inner_iteration_tolerance): blocks = "automatic", "cameras", "points", "cameras,points", "points,cameras" (bundle_adjuster's
        --blocks_for_inner_iterations) or None (off) — or an INNER_* number.  In force until set again."""
        if blocks is None or isinstance(blocks, str):
            if blocks not in INNER_BLOCKS:
                raise ValueError(f"unknown blocks {blocks!r}: one of {', '.join(str(k) for k in INNER_BLOCKS)}")
            blocks = INNER_BLOCKS[blocks]
        self._check(self._lib.ceres_hip_bal_set_inner_iterations(self._h, int(blocks), float(tolerance)))

    def set_trust_region_strategy(self, strategy="levenberg_marquardt", dogleg="traditional"):
        """Solver::Options::trust_region_strategy_type and dogleg_type (bundle_adjuster --trust_region_strategy, --dogleg):
        strategy = "levenberg_marquardt" or "dogleg", dogleg = "traditional" or "subspace" (read with "dogleg" only) — or the numbers.
        DOGLEG needs an exact factorisation (DENSE_SCHUR here).  In force for later minimize calls until set again."""
        if isinstance(strategy, str):
            if strategy not in TRUST_REGION_STRATEGIES:
                raise ValueError(f"unknown strategy {strategy!r}: one of {', '.join(TRUST_REGION_STRATEGIES)}")
            strategy = TRUST_REGION_STRATEGIES[strategy]
        if isinstance(dogleg, str):
            if dogleg not in DOGLEG_TYPES:
                raise ValueError(f"unknown dogleg type {dogleg!r}: one of {', '.join(DOGLEG_TYPES)}")
            dogleg = DOGLEG_TYPES[dogleg]
        self._check(self._lib.ceres_hip_bal_set_trust_region_strategy(self._h, int(strategy), int(dogleg)))

    def inner_iterate(self, state):
        """One coordinate-descent pass at state.  Returns (state, cost_before, cost_after, block_iterations: per block in state order, -1
        outside the ordering)."""
        x = _f64(state, self.num_parameters).copy()
        c0, c1 = np.zeros(1), np.zeros(1)
        its = np.empty(self.num_points + self.num_cameras, dtype=np.int32)
        self._check(self._lib.ceres_hip_bal_inner_iterate(self._h, _p(x), _p(c0), _p(c1), its.ctypes.data_as(POINTER(c_int32))))
        return x, float(c0[0]), float(c1[0]), its

    def inner_iteration_stats(self):
        """Of the last minimize: (num_inner_iteration_steps, inner_iteration_seconds, groups of the ordering)."""
        n, t, g = c_int32(), np.zeros(1), c_int32()
        self._check(self._lib.ceres_hip_bal_inner_iteration_stats(self._h, byref(n), _p(t), byref(g)))
        return n.value, float(t[0]), g.value

    def evaluate(self, state, residuals=False, gradient=False, jacobian=False):
        """Evaluator::Evaluate: returns (cost, residuals|None, gradient|None, jacobian values|None); the gradient and the Jacobian are
        the local (tangent) ones."""
        x = _f64(state, self.num_parameters)
        cost = np.zeros(1)
        r = np.empty(self.num_residuals) if residuals else None
        g = np.empty(self.num_effective_parameters) if gradient else None
        v = np.empty(self.num_jacobian_values) if jacobian else None
        self._check(self._lib.ceres_hip_bal_evaluate(self._h, _p(x), _p(cost), _p(r), _p(g), _p(v)))
        return float(cost[0]), r, g, v

    def minimize(self, state, **opts):
        """TrustRegionMinimizer::Minimize (LEVENBERG_MARQUARDT, or what set_trust_region_strategy chose).  Returns (state, CMinimizerSummary)."""
        o = CMinimizerOptions()
        self._lib.ceres_hip_minimizer_default_options(byref(o))
        for k, val in opts.items():
            if not hasattr(o, k):
                raise TypeError(f"unknown minimizer option {k}")
            setattr(o, k, val)
        x = _f64(state, self.num_parameters).copy()
        S = CMinimizerSummary()
        self._check(self._lib.ceres_hip_bal_minimize(self._h, byref(o), _p(x), byref(S)))
        return x, S

    def set_bounds(self, lower=None, upper=None, **line_search_options_):
        """Problem::SetParameterLowerBound / SetParameterUpperBound for every coordinate of the state at once (num_parameters doubles
        each; None: no bound on that side, both None: clears).  The keyword arguments are the line-search fields of the projected search
        (line_search_interpolation_type, min_line_search_step_size, line_search_sufficient_function_decrease,
        max/min_line_search_step_contraction, max_num_line_search_step_size_iterations).  In force until set again."""
        lo = None if lower is None else _f64(lower, self.num_parameters)
        hi = None if upper is None else _f64(upper, self.num_parameters)
        o = line_search_options(**line_search_options_) if line_search_options_ else None
        self._check(self._lib.ceres_hip_bal_set_bounds(self._h, _p(lo), _p(hi), byref(o) if o is not None else None))

    def project(self, state):
        """Program::Plus(state, 0): (the state clamped to the bounds on the free blocks, the number of coordinates moved)."""
        x = _f64(state, self.num_parameters).copy()
        n = c_int64()
        self._check(self._lib.ceres_hip_bal_project(self._h, _p(x), byref(n)))
        return x, n.value

    def bounds_stats(self):
        """Of the last minimize: dict(is_constrained, num_line_search_steps, num_function_evaluations, num_gradient_evaluations,
        line_search_seconds, num_projected, and per logged iteration line_search_iterations (-1: none ran), line_search_success,
        step_size)."""
        c, n, f, g, m = c_int32(), c_int32(), c_int32(), c_int32(), c_int64()
        t = np.zeros(1)
        its, ok = np.empty(MAX_LOGGED_ITERATIONS, dtype=np.int32), np.empty(MAX_LOGGED_ITERATIONS, dtype=np.int32)
        step = np.empty(MAX_LOGGED_ITERATIONS)
        self._check(self._lib.ceres_hip_bal_bounds_stats(self._h, byref(c), byref(n), byref(f), byref(g), _p(t), byref(m),
                                                         its.ctypes.data_as(POINTER(c_int32)), ok.ctypes.data_as(POINTER(c_int32)), _p(step)))
        return dict(is_constrained=c.value, num_line_search_steps=n.value, num_function_evaluations=f.value,
                    num_gradient_evaluations=g.value, line_search_seconds=float(t[0]), num_projected=m.value,
                    line_search_iterations=its, line_search_success=ok, step_size=step)

    def bounded_step(self, state, v, t):
        """Debug: the bounded loop's vector kernels at a state.  v: tangent (num_effective_parameters).  Returns (clamp(state + t v) on
        the free blocks, |state| and |trial - state| over the free blocks, max |state - clamp(state - v)|)."""
        x = _f64(state, self.num_parameters)
        d = _f64(v, self.num_effective_parameters)
        out = np.empty(self.num_parameters)
        xn, sn, pm = np.zeros(1), np.zeros(1), np.zeros(1)
        self._check(self._lib.ceres_hip_debug_bal_bounded_step(self._h, _p(x), _p(d), float(t), _p(out), _p(xn), _p(sn), _p(pm)))
        return out, float(xn[0]), float(sn[0]), float(pm[0])

    def evaluate_gradient(self, state, gradient=True):
        """Evaluator::Evaluate(state, cost, nullptr, gradient, nullptr) without a Jacobian in memory: (cost, tangent gradient | None)."""
        x = _f64(state, self.num_parameters)
        cost = np.zeros(1)
        g = np.empty(self.num_effective_parameters) if gradient else None
        self._check(self._lib.ceres_hip_bal_evaluate_gradient(self._h, _p(x), _p(cost), _p(g)))
        return float(cost[0]), g

    def minimize_line_search(self, state, **opts):
        """LineSearchMinimizer::Minimize (L-BFGS with a Wolfe line search by default).  Returns (state, CLineSearchSummary)."""
        o = line_search_options(**opts)
        x = _f64(state, self.num_parameters).copy()
        S = CLineSearchSummary()
        self._check(self._lib.ceres_hip_bal_minimize_line_search(self._h, byref(o), _p(x), byref(S)))
        return x, S

    def covariance_block_size(self, block):
        """Tangent size of a block numbered in state order (point q is q, camera c is num_points + c): 3, or 9 / 10 for a camera.  With
        camera_groups camera c's block is its POSE (6) and group g is block num_points + num_cameras + g (3)."""
        if block < self.num_points:
            return 3
        if self.num_intrinsics_groups:
            return 6 if block < self.num_points + self.num_cameras else 3
        return 10 if self.camera_model == CAMERA_QUATERNION else 9

    @property
    def num_covariance_blocks(self):
        """How many blocks ceres_hip_bal_covariance numbers: the points, the cameras and, with camera_groups, the groups behind them."""
        return self.num_points + self.num_cameras + self.num_intrinsics_groups

    def covariance_raw(self, state, pairs, apply_loss_function=True, min_scaled_pivot=1e-8, out=None):
        """ceres_hip_bal_covariance without judging the outcome: (return code, flat output, CCovarianceSummary).  `out` (optional): the
        flat output array to fill, at least the sum of dim(a) x dim(b) doubles; it is left as it is when the call fails.  Blocks are
        numbered as `covariance_block_size` says (with camera_groups: points, poses, then the groups)."""
        x = _f64(state, self.num_parameters)
        pr = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        a, b = np.ascontiguousarray(pr[:, 0]), np.ascontiguousarray(pr[:, 1])
        nblocks = self.num_covariance_blocks
        # (sizes of in-range blocks only: an index out of range is the library's to refuse)
        total = sum(self.covariance_block_size(int(i)) * self.covariance_block_size(int(j)) for i, j in pr
                    if 0 <= i < nblocks and 0 <= j < nblocks)
        if out is None:
            out = np.zeros(max(total, 1))
        elif out.dtype != np.float64 or not out.flags.c_contiguous or out.size < total:
            raise ValueError("out must be a contiguous float64 array with room for every requested block")
        o = CCovarianceOptions()
        self._lib.ceres_hip_covariance_default_options(byref(o))
        o.apply_loss_function = int(bool(apply_loss_function))
        o.min_scaled_pivot = float(min_scaled_pivot)
        S = CCovarianceSummary()
        rc = self._lib.ceres_hip_bal_covariance(self._h, byref(o), _p(x), int(pr.shape[0]), a.ctypes.data_as(POINTER(c_int32)),
                                                b.ctypes.data_as(POINTER(c_int32)), _p(out), byref(S))
        return rc, out, S

    def covariance(self, state, pairs, apply_loss_function=True, min_scaled_pivot=1e-8):
        """ceres::Covariance::Compute + GetCovarianceBlockInTangentSpace for the (a, b) block pairs (state order: point q is q, camera c
        is num_points + c): (J^T J)^-1 of the reduced program at state, in the Schur form on the device (DENSE_SCHUR handles only).
        With camera_groups the columns are [points | poses of the free cameras | groups]: camera c's block is its 6-wide pose, group g
        is block num_points + num_cameras + g (3 wide, never constant), and a pair with a constant pose is zeros.
        Returns (list of dim(a) x dim(b) arrays, CCovarianceSummary); pairs with a constant block are zeros.  Raises HipError with the
        summary's message when the problem is rank deficient (a pivot of the unit-diagonal-scaled point blocks or Schur complement is
        not above min_scaled_pivot) — ceres_hip_bal_covariance in include/ceres_hip.h."""
        rc, out, S = self.covariance_raw(state, pairs, apply_loss_function, min_scaled_pivot)
        self._check(rc)
        if S.termination_type != SUCCESS:
            raise HipError(S.message.decode())
        blocks, at = [], 0
        for i, j in np.asarray(pairs, dtype=np.int64).reshape(-1, 2):
            da, db = self.covariance_block_size(int(i)), self.covariance_block_size(int(j))
            blocks.append(out[at:at + da * db].reshape(da, db).copy())
            at += da * db
        return blocks, S
