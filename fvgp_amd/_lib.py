"""ctypes binding of libfvgp_hip.so (include/fvgp_hip.h) -- the only door into the HIP kernels.

There is no CPU fallback: if the shared library is missing or a call fails, this module
raises.  `build()` compiles the library in-tree with hipcc for gfx950 (works without a GPU).
"""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIB_PATH = os.environ.get("FVGP_HIP_LIB", os.path.join(CSRC, "libfvgp_hip.so"))     # FVGP_HIP_LIB: A/B another build of the same ABI

KERNEL_IDS = {"rbf_ard": 0, "matern32_ard": 1, "matern52_ard": 2,
              "rbf_iso": 3, "matern32_iso": 4, "matern52_iso": 5}
_ISO_IDS = frozenset(v for k, v in KERNEL_IDS.items() if k.endswith("_iso"))
FULL, LOWER = 0, 1
PAD_NONE, PAD_IDENTITY, PAD_ZERO = 0, 1, 2
TILE = 128
MAX_RHS_VEC = 8

MATVEC_CHUNK = 4096       # FVGP_MATVEC_CHUNK: rows of x2 per chunk sum of fvgp_hip_kmatvec
PCG_MAX_RHS = 16          # FVGP_PCG_MAX_RHS
PCG_MAX_RANK = 1024       # FVGP_PCG_MAX_RANK
LANCZOS_MAX_STEPS = 256   # FVGP_LANCZOS_MAX_STEPS: most CG coefficients per column fvgp_hip_pcg_lanczos records
CHOL_UPDATE_MAX_RANK = 16 # FVGP_CHOL_UPDATE_MAX_RANK: columns of W per pass of fvgp_hip_chol_update
CHOL_UPDATE_TABLE_BYTES = 128 * CHOL_UPDATE_MAX_RANK * 2 * 8   # FVGP_CHOL_UPDATE_TABLE_BYTES: all of the workspace the update itself uses
BATCH_MAX_DIM = 4096      # FVGP_BATCH_MAX_DIM: largest per-problem square fvgp_hip_loglik_batch takes
# options a new Handle takes from the environment, FVGP_<KEY>=<integer> (tuning overrides, e.g. FVGP_OUTER_BLOCK=512)
OPTION_KEYS = (
    "schedule", "lookahead", "outer_block", "outer_block_big", "big_threshold", "inner_block", "small_tile_max", "small_tile_max_update",
    "tile_tables", "block_inverses", "k128_kernels", "leaf_tiles", "leaf_tiles_rows", "panel_recursive", "potri_kminor", "leaf_yield",
    "chain_yield", "lookahead_min", "posterior_halves", "posterior_block", "outer_block_small", "small_threshold", "panel_chain",
    "panel_chain_min", "cols_split", "cols_split_rows", "bwd_sweep", "fwd_sweep", "chain_verify", "chain_wide", "wide_block",
    "wide_block_big", "wide_threshold", "wide_inner", "wide_inner_rows", "chain_sleep_rows", "chain_single_rows", "chain_ahead",
    "select_block", "matvec_split")


# ---- the C ABI as ctypes sees it: structures and signatures of include/fvgp_hip.h ------------------------------------
# device pointers are c_void_p (callers pass _ptr(tensor) or None), host out-parameters typed POINTERs (callers pass ctypes arrays,
# byref() or ndarray.ctypes.data_as)
c_i, c_l, c_u, c_d = ctypes.c_int, ctypes.c_int64, ctypes.c_uint64, ctypes.c_double
c_p, c_s = ctypes.c_void_p, ctypes.c_char_p
P_i, P_l, P_d, P_p, P_u32 = (ctypes.POINTER(t) for t in (c_i, c_l, c_d, c_p, ctypes.c_uint32))

ALL_GATHER_FN = ctypes.CFUNCTYPE(c_i, c_p, c_p, c_p, c_l, c_p)
ALL_REDUCE_FN = ctypes.CFUNCTYPE(c_i, c_p, c_p, c_l, c_p)


class Collectives(ctypes.Structure):
    _fields_ = [("ctx", c_p), ("all_gather", ALL_GATHER_FN), ("all_reduce_sum", ALL_REDUCE_FN)]


class DistDesc(ctypes.Structure):
    _fields_ = [("n", c_l), ("d", c_i), ("ncol", c_i), ("panel", c_l), ("rank", c_i), ("nranks", c_i), ("kernel_id", c_i),
                ("x_all", c_p), ("vdiag", c_p), ("zt", c_p), ("A", c_p), ("T", c_p * 2), ("recv", c_p * 2), ("Dfac", c_p),
                ("gather", c_p), ("info_dev", c_p), ("logdet_dev", c_p),
                ("keep_factor", c_i), ("force_general", c_i), ("preassembled", c_i)]


P_coll, P_desc = ctypes.POINTER(Collectives), ctypes.POINTER(DistDesc)
_PCG_ARGS = [c_p, c_i, c_p, c_l, c_i, P_d, c_i, c_p, c_p, c_l, c_i, c_p, c_l, c_p, c_l, c_i, c_p, c_l, c_i, c_d, c_i, c_i, c_i,
             c_p, c_l, P_i, P_d, P_i]
# the sparse nearest-neighbour factor as fvgp_hip_nn_precond_apply and fvgp_hip_pcg_nn take it: idx, ld, m, coef, dinv, tr_start, tr_pos, nnz
_NN_FACTOR_ARGS = [c_p, c_l, c_i, c_p, c_p, c_p, c_p, c_l]

# name -> (restype, [argtypes]) for every prototype of include/fvgp_hip.h, in the header's order under its section comments
# (tests/test_host_logic.py::test_abi_table_matches_header parses the header and holds this table to it)
_ABI = {
    "fvgp_hip_version": (c_i, []),
    "fvgp_hip_last_error_string": (c_s, []),
    "fvgp_hip_padded_dim": (c_l, [c_l]),
    "fvgp_hip_loglik_dim": (c_l, [c_l, c_i]),
    "fvgp_hip_workspace_bytes": (c_l, [c_l, c_l]),
    "fvgp_hip_create": (c_i, [P_p, c_i, c_p]),
    "fvgp_hip_destroy": (c_i, [c_p]),
    "fvgp_hip_sync": (c_i, [c_p]),
    "fvgp_hip_stream_create": (c_i, [P_p, c_i, c_i, P_u32, c_i]),
    "fvgp_hip_stream_destroy": (c_i, [c_p]),
    "fvgp_hip_set_option": (c_i, [c_p, c_s, c_l]),
    "fvgp_hip_chain_verify_counts": (c_i, [c_p, P_l]),
    "fvgp_hip_get_profile": (c_i, [c_p, P_d]),
    "fvgp_hip_get_profile_ex": (c_i, [c_p, P_d]),
    "fvgp_hip_invalidate_factor": (c_i, [c_p]),
    # ---- covariance assembly
    "fvgp_hip_kmat": (c_i, [c_p, c_i, c_p, c_l, c_p, c_l, c_i, P_d, c_i, c_p, c_p, c_l, c_i, c_i]),
    # ---- dense Cholesky
    "fvgp_hip_potrf": (c_i, [c_p, c_p, c_l, c_l, P_i]),
    "fvgp_hip_potrf_dev": (c_i, [c_p, c_p, c_l, c_l, c_l, c_p, c_p]),
    "fvgp_hip_potrs": (c_i, [c_p, c_p, c_l, c_l, c_p, c_l, c_l]),
    "fvgp_hip_logdet": (c_i, [c_p, c_p, c_l, c_l, P_d]),
    "fvgp_hip_potri": (c_i, [c_p, c_p, c_l, c_l, c_p, c_l]),
    "fvgp_hip_trsm_lower": (c_i, [c_p, c_p, c_l, c_l, c_p, c_l, c_l]),
    "fvgp_hip_trsm_lower_t": (c_i, [c_p, c_p, c_l, c_l, c_p, c_l, c_l]),
    # ---- row-sharded (multi-GPU) building blocks: the gp2Scale partitioning pattern
    "fvgp_hip_panel_trsm": (c_i, [c_p, c_p, c_l, c_l, c_p, c_l, c_l]),
    # ---- row-sharded (multi-GPU) evaluation: one process per GPU, RCCL over xGMI
    "fvgp_hip_comm_unique_id": (c_i, [c_p]),
    "fvgp_hip_comm_init": (c_i, [c_p, c_p, c_i, c_i]),
    "fvgp_hip_comm_init_callbacks": (c_i, [c_p, P_coll, c_i, c_i]),
    "fvgp_hip_comm_destroy": (c_i, [c_p]),
    "fvgp_hip_ipc_window": (c_i, [c_p, c_l, c_p]),
    "fvgp_hip_comm_init_ipc": (c_i, [c_p, c_p, c_s, c_i, c_i]),
    "fvgp_hip_all_reduce": (c_i, [c_p, c_p, c_l]),
    "fvgp_hip_all_gather": (c_i, [c_p, c_p, c_p, c_l]),
    "fvgp_hip_comm_profile": (c_i, [c_p, P_d]),
    "fvgp_hip_comm_info": (c_i, [c_p, P_l]),
    "fvgp_hip_comm_check": (c_i, [c_p]),
    "fvgp_hip_dist_workspace": (c_i, [P_desc, P_l]),
    "fvgp_hip_loglik_dist": (c_i, [c_p, P_desc, P_d, c_i, P_d, P_i]),
    "fvgp_hip_dist_scratch": (c_l, [P_desc, c_i, c_l, c_l]),
    "fvgp_hip_solve_dist": (c_i, [c_p, P_desc, c_p, c_p]),
    "fvgp_hip_posterior_dist": (c_i, [c_p, P_desc, P_d, c_i, c_p, c_l, c_p, c_p, c_p, c_p, c_p, c_p]),
    "fvgp_hip_grad_dist": (c_i, [c_p, P_desc, P_d, c_i, c_p, c_i, c_l, P_d, c_p, c_p]),
    "fvgp_hip_panel_potrf_dev": (c_i, [c_p, c_p, c_l, c_l, c_l, c_l, c_p, c_p]),
    "fvgp_hip_syrk_rowshard": (c_i, [c_p, c_l, c_l, c_l, c_p, c_l, c_p, c_l, c_p, c_l, c_i, c_i, c_i, c_i, c_i]),
    # ---- fused evaluations
    "fvgp_hip_loglik": (c_i, [c_p, c_i, c_p, c_l, c_i, P_d, c_i, c_p, c_p, c_i, c_p, c_l, c_p, P_d, P_i]),
    "fvgp_hip_loglik_rows": (c_i, [c_p, c_i, c_p, c_l, c_i, P_d, c_i, c_p, c_p, c_i, c_p, c_l, c_l, c_p, P_d, P_i]),
    "fvgp_hip_loglik_batch": (c_i, [c_p, c_i, c_p, c_l, c_i, P_d, c_i, c_l, c_p, c_l, c_p, c_l, c_i, c_p, c_l, c_l, P_d, P_i]),
    "fvgp_hip_loglik_batch_dim": (c_l, [c_l, c_i]),
    "fvgp_hip_loglik_batch_workspace_bytes": (c_l, [c_l, c_i, c_l]),
    "fvgp_hip_loglik_grad_batch": (c_i, [c_p, c_i, c_p, c_l, c_i, P_d, c_i, c_l, c_p, c_l, c_p, c_l, c_i, c_i, c_p, c_l, c_l,
                                         c_p, c_l, c_l, P_d, P_d, P_i, c_p, c_p]),
    "fvgp_hip_loglik_grad_batch_workspace_bytes": (c_l, [c_l, c_i, c_l]),
    "fvgp_hip_posterior_batch": (c_i, [c_p, c_i, c_p, c_l, c_i, P_d, c_i, c_l, c_p, c_l, c_p, c_l, c_i, c_p, c_l,
                                       c_p, c_l, c_l, c_l, c_p, c_p, c_p, c_l, c_l, P_d, P_i]),
    "fvgp_hip_posterior_batch_workspace_bytes": (c_l, [c_l, c_i, c_l, c_l]),
    "fvgp_hip_loglik_grad": (c_i, [c_p, c_i, c_p, c_l, c_i, P_d, c_i, c_p, c_i, c_i, c_p, c_l, c_p, c_l, P_d]),
    "fvgp_hip_loglik_hess_workspace_bytes": (c_l, [c_l, c_i]),
    "fvgp_hip_loglik_hess": (c_i, [c_p, c_i, c_p, c_l, c_i, P_d, c_i, c_p, c_i, c_i, c_p, c_l, c_p, c_l, c_p, c_l, c_p, c_l, P_d, P_d]),
    "fvgp_hip_grad_trace": (c_i, [c_p, c_i, c_p, c_l, c_i, P_d, c_i, c_p, c_l, c_p, c_l, c_p, P_d]),
    "fvgp_hip_grad_trace_cols": (c_i, [c_p, c_i, c_p, c_l, c_i, P_d, c_i, c_p, c_l, c_l, c_l, c_p, c_l, c_p, P_d]),
    "fvgp_hip_posterior_prepare": (c_i, [c_p, c_p, c_l, c_l]),
    "fvgp_hip_posterior": (c_i, [c_p, c_i, c_p, c_l, c_i, P_d, c_i, c_p, c_l, c_p, c_i, c_p, c_l, c_p, c_l, c_p, c_p, c_p, c_l]),
    "fvgp_hip_posterior_grad": (c_i, [c_p, c_i, c_p, c_l, c_i, P_d, c_i, c_p, c_l, c_p, c_i, c_i, c_p, c_l, c_i,
                                      c_p, c_l, c_p, c_p, c_p, c_p]),
    "fvgp_hip_posterior_grad_workspace_bytes": (c_l, [c_l, c_l, c_i]),
    "fvgp_hip_potrs_cols": (c_i, [c_p, c_p, c_l, c_l, c_p, c_l, c_l]),
    "fvgp_hip_loo": (c_i, [c_p, c_i, c_p, c_l, c_i, P_d, c_i, c_p, c_i, c_i, c_p, c_l, c_p, c_l, c_p, c_l,
                           P_d, c_p, c_p, P_d, c_p, c_p]),
    "fvgp_hip_loo_workspace_bytes": (c_l, [c_l]),
    # ---- sampling
    "fvgp_hip_normal_fill": (c_i, [c_p, c_u, c_u, c_l, c_l, c_p, c_l, c_l, c_l]),
    "fvgp_hip_mvn_sample": (c_i, [c_p, c_p, c_l, c_l, c_p, c_u, c_u, c_l, c_l, c_p, c_l, c_p, c_l, c_p, c_l]),
    "fvgp_hip_select_batch": (c_i, [c_p, c_i, c_p, c_l, c_i, P_d, c_i, c_p, c_l, c_p, c_l, c_p, c_p, c_i, c_i, c_i, c_d,
                                    c_p, c_l, c_p, c_p, c_p, c_l]),
    "fvgp_hip_select_workspace_bytes": (c_l, [c_l, c_l, c_i]),
    "fvgp_hip_mvn_sample_workspace_bytes": (c_l, [c_l, c_l]),
    # ---- matrix-free solves
    "fvgp_hip_kmatvec": (c_i, [c_p, c_i, c_p, c_l, c_p, c_l, c_i, P_d, c_i, c_p, c_p, c_l, c_i, c_p, c_l, c_p, c_l]),
    "fvgp_hip_kmatvec_workspace_bytes": (c_l, [c_l, c_l, c_i]),
    "fvgp_hip_pchol": (c_i, [c_p, c_i, c_p, c_l, c_i, P_d, c_i, c_i, c_d, c_p, c_l, c_p, c_p, c_p, c_l, P_i]),
    "fvgp_hip_pchol_workspace_bytes": (c_l, [c_l, c_i]),
    "fvgp_hip_precond_factor": (c_i, [c_p, c_p, c_l, c_i, c_l, c_p, c_p, c_l, c_p, c_l, P_i]),
    "fvgp_hip_precond_workspace_bytes": (c_l, [c_l, c_i]),
    "fvgp_hip_pcg": (c_i, _PCG_ARGS),
    "fvgp_hip_pcg_workspace_bytes": (c_l, [c_l, c_i]),
    # ---- the stochastic log-likelihood on the matrix-free path
    "fvgp_hip_kgrad_form": (c_i, [c_p, c_i, c_p, c_l, c_p, c_l, c_i, P_d, c_i, c_p, c_l, c_p, c_l, c_i, c_p, c_l, P_d]),
    "fvgp_hip_kgrad_form_workspace_bytes": (c_l, [c_l, c_l]),
    "fvgp_hip_precond_probes": (c_i, [c_p, c_u, c_u, c_l, c_p, c_l, c_i, c_l, c_p, c_p, c_l, c_i]),
    "fvgp_hip_precond_apply": (c_i, [c_p, c_p, c_l, c_i, c_p, c_l, c_l, c_p, c_p, c_l, c_i, c_p, c_l, c_p, c_l]),
    "fvgp_hip_precond_apply_workspace_bytes": (c_l, [c_l, c_i]),
    "fvgp_hip_pcg_lanczos": (c_i, _PCG_ARGS + [c_i, P_d, P_d, P_i, P_d]),
    "fvgp_hip_pcg_lanczos_workspace_bytes": (c_l, [c_l, c_i, c_i]),
    # ---- rank-k update of a resident factor, removal of data points
    "fvgp_hip_chol_update": (c_i, [c_p, c_p, c_l, c_l, c_p, c_l, c_l, c_l, c_p, c_l]),
    "fvgp_hip_chol_delete": (c_i, [c_p, c_p, c_l, c_l, P_l, c_l, c_p, c_l]),
    "fvgp_hip_chol_update_workspace_bytes": (c_l, [c_l, c_l]),
    # ---- building blocks exported for the parity tests
    "fvgp_hip_gemm": (c_i, [c_p, c_i, c_i, c_i, c_l, c_l, c_l, c_d, c_p, c_l, c_p, c_l, c_d, c_p, c_l]),
    "fvgp_hip_mfma_selftest": (c_i, [c_p, c_p, c_p, c_p]),
    "fvgp_hip_debug_tile_map": (c_l, [c_i, c_i, c_i, c_i, c_i, P_i, P_i, c_l]),
    "fvgp_hip_debug_tile_table": (c_l, [c_i, c_i, c_i, c_i, c_i, P_i, c_l]),
    "fvgp_hip_debug_chain_ticket": (c_i, [c_i, c_i, c_i, c_i, P_i]),
    "fvgp_hip_mfma_peak": (c_i, [c_p, c_p, c_i, c_i]),
    "fvgp_hip_add_lower": (c_i, [c_p, c_p, c_l, c_l, c_p, c_l, c_d]),
    "fvgp_hip_trace_dot": (c_i, [c_p, c_p, c_l, c_p, c_l, c_p, c_l, c_l, P_d]),
    "fvgp_hip_dot": (c_i, [c_p, c_p, c_l, c_p, c_l, c_l, c_i, P_d]),
    "fvgp_hip_coldot": (c_i, [c_p, c_p, c_l, c_p, c_l, c_l, c_l, c_p]),
    "fvgp_hip_colsumsq": (c_i, [c_p, c_p, c_l, c_l, c_l, c_p]),
    "fvgp_hip_add_matrix": (c_i, [c_p, c_p, c_l, c_p, c_l, c_l, c_l, c_d]),
    "fvgp_hip_symmetrize": (c_i, [c_p, c_p, c_l, c_l]),
}
SYMBOLS = list(_ABI)      # every symbol include/fvgp_hip.h declares (tests check the library exports each of them)

# the same for include/fvgp_hip_nn.h, the nearest-neighbour (Vecchia) entries (tests/test_vecchia_host.py holds this table to that header)
_ABI_NN = {
    "fvgp_hip_nn_search": (c_i, [c_p, c_p, c_l, c_p, c_l, c_i, P_d, c_i, c_l, c_p, c_l]),
    "fvgp_hip_nn_conditionals": (c_i, [c_p, c_i, c_p, c_l, c_p, c_l, c_i, P_d, c_i, c_i, c_p, c_l, c_i, c_p, c_p, c_p, c_p, c_p,
                                       c_p, c_l, P_l]),
    "fvgp_hip_nn_loglik": (c_i, [c_p, c_i, c_p, c_l, c_i, P_d, c_i, c_i, c_p, c_l, c_i, c_p, c_p, c_p, c_p, c_p, c_l, P_d, P_l]),
    "fvgp_hip_nn_workspace_bytes": (c_l, [c_i, c_l, c_i]),
    "fvgp_hip_nn_loglik_grad": (c_i, [c_p, c_i, c_p, c_l, c_i, P_d, c_i, c_i, c_p, c_l, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_l, P_d, P_d,
                                      P_l]),
    "fvgp_hip_nn_grad_workspace_bytes": (c_l, [c_l, c_i, c_i]),
    "fvgp_hip_nn_loglik_fisher": (c_i, [c_p, c_i, c_p, c_l, c_i, P_d, c_i, c_i, c_p, c_l, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_l, P_d,
                                        P_d, P_d, P_l]),
    "fvgp_hip_nn_fisher_workspace_bytes": (c_l, [c_l, c_i, c_i]),
    "fvgp_hip_nn_grid_bytes": (c_l, [c_l, c_i]),
    "fvgp_hip_nn_grid_workspace_bytes": (c_l, [c_l, c_i]),
    "fvgp_hip_nn_grid_build": (c_i, [c_p, c_p, c_l, c_i, P_d, c_p, c_l, c_p, c_l, P_d]),
    "fvgp_hip_nn_grid_search": (c_i, [c_p, c_p, c_l, c_p, c_l, c_i, c_i, c_l, P_d, c_p, c_p, c_l]),
    # ---- the nearest-neighbour factor as the matrix-free solves' preconditioner
    "fvgp_hip_nn_factor_workspace_bytes": (c_l, [c_l]),
    "fvgp_hip_nn_factor": (c_i, [c_p, c_i, c_p, c_l, c_i, P_d, c_i, c_p, c_l, c_i, c_p, c_p, c_l, c_p, c_p, c_l, P_l]),
    "fvgp_hip_nn_precond_apply_workspace_bytes": (c_l, [c_l]),
    "fvgp_hip_nn_precond_apply": (c_i, [c_p, c_l] + _NN_FACTOR_ARGS + [c_p, c_l, c_i, c_p, c_l, c_p, c_l]),
    "fvgp_hip_pcg_nn_workspace_bytes": (c_l, [c_l]),
    "fvgp_hip_pcg_nn": (c_i, _PCG_ARGS[:8] + _NN_FACTOR_ARGS + _PCG_ARGS[13:]),
    "fvgp_hip_nn_maxmin_workspace_bytes": (c_l, [c_l]),
    "fvgp_hip_nn_maxmin_order": (c_i, [c_p, c_p, c_l, c_i, P_d, c_l, c_l, c_p, c_p, c_p, c_l]),
}
SYMBOLS_NN = list(_ABI_NN)
NN_MAX_NEIGHBORS = 64     # FVGP_NN_MAX_NEIGHBORS
NN_GRID_MAX_DIM = 3       # FVGP_NN_GRID_MAX_DIM: most dimensions of the cell-grid search
NN_GRID_INFO = 20         # FVGP_NN_GRID_INFO: doubles of the host record a grid build leaves for the grid search
NN_SEARCH, NN_CONDITIONALS, NN_LOGLIK = 0, 1, 2   # FVGP_NN_*: the call fvgp_hip_nn_workspace_bytes sizes
NN_VALUE, NN_GRAD, NN_FISHER = 0, 1, 2            # how far a likelihood call goes: fvgp_hip_nn_loglik, _loglik_grad, _loglik_fisher


def bind(L):
    """set restype and argtypes of every entry of _ABI and _ABI_NN that the loaded library `L` exports (libfvgp_hip.so exports all of
    them; the tests bind the CPU twin of the ABI, which implements a subset, the same way); returns L"""
    for table in (_ABI, _ABI_NN):
        for name, (restype, argtypes) in table.items():
            if hasattr(L, name):
                fn = getattr(L, name)
                fn.restype, fn.argtypes = restype, list(argtypes)
    return L


bind_dist = bind          # the name the row-sharded tests' CPU stand-in binds through


class DistCalls:
    """The row-sharded entry points that follow a kept factorisation (include/fvgp_hip.h: fvgp_hip_solve_dist, _posterior_dist,
    _grad_dist), as methods over `self._dist_lib()` (the loaded library) and `self._h` (its handle) with `self._dist_check` as the
    status check: the product's Handle binds libfvgp_hip.so, the CPU tests' stand-in binds the CPU twin of the ABI the same way.
    Tensors are anything with data_ptr()."""

    def dist_scratch(self, desc, what, npred=0, slab=TILE):
        n = self._dist_lib().fvgp_hip_dist_scratch(ctypes.byref(desc), int(what), int(npred), int(slab))
        if n < 0:
            raise ValueError("fvgp_hip_dist_scratch: bad arguments")
        return int(n)

    def solve_dist(self, desc, alpha_out, ws):
        self._dist_check(self._dist_lib().fvgp_hip_solve_dist(self._h, ctypes.byref(desc), _ptr(alpha_out), _ptr(ws)), "fvgp_hip_solve_dist")

    def posterior_dist(self, desc, theta, xpred, npred, k_pre, kk_pre, alpha, mean_out, S_out, ws):
        t, tp, nt = _theta(theta)
        self._dist_check(self._dist_lib().fvgp_hip_posterior_dist(self._h, ctypes.byref(desc), tp, nt, _ptr(xpred), int(npred), _ptr(k_pre), _ptr(kk_pre),
                                                                  _ptr(alpha), _ptr(mean_out), _ptr(S_out), _ptr(ws)), "fvgp_hip_posterior_dist")

    def grad_dist(self, desc, theta, alpha, component, slab, diag_out, ws):
        t, tp, nt = _theta(theta)
        g = (ctypes.c_double * nt)()
        self._dist_check(self._dist_lib().fvgp_hip_grad_dist(self._h, ctypes.byref(desc), tp, nt, _ptr(alpha), int(component), int(slab), g,
                                                             _ptr(diag_out), _ptr(ws)), "fvgp_hip_grad_dist")
        return np.array(list(g))


class HipExtensionError(RuntimeError):
    """The native library is missing, failed to load, or a call into it failed."""


def build(force=False, verbose=False):
    """Compile fvgp_amd/csrc/*.hip into libfvgp_hip.so (hipcc --offload-arch=gfx950)."""
    cmd = ["make", "-C", CSRC, "-j4"]
    if force:
        subprocess.run(["make", "-C", CSRC, "clean"], check=True, capture_output=not verbose)
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise HipExtensionError("building libfvgp_hip.so failed:\n" + res.stdout[-4000:] + res.stderr[-4000:])
    if verbose:
        print(res.stdout[-2000:])
    return LIB_PATH


_lib = None


def pad128(n):
    return (int(n) + TILE - 1) // TILE * TILE


def loglik_dim(n, ncol=1):
    """rows and columns of the square scratch the fused evaluation wants (fvgp_hip_loglik_dim): padded_dim(n), or 128 more when n
    leaves fewer than ncol padding rows for the appended (y-m)^T"""
    n, ncol = int(n), int(ncol)
    return pad128(n) if pad128(n) - n >= ncol else pad128(n + ncol)


def loglik_batch_dim(n, ncol=1):
    """rows = columns of one problem's square in the batched scratch (fvgp_hip_loglik_batch_dim): loglik_dim(n, ncol), 0 past
    BATCH_MAX_DIM"""
    d = loglik_dim(n, ncol)
    return d if d <= BATCH_MAX_DIM else 0


def _workspace_bytes(name, *sizes):
    """the *_workspace_bytes query `name` of the library at integer arguments"""
    return int(getattr(lib(), name)(*map(int, sizes)))


def posterior_batch_workspace_bytes(n, ncol, B, P_chunk):
    """device bytes the handle allocates for Handle.posterior_batch (fvgp_hip_posterior_batch_workspace_bytes); <= 0: invalid arguments"""
    return _workspace_bytes("fvgp_hip_posterior_batch_workspace_bytes", n, ncol, B, P_chunk)


def posterior_grad_workspace_bytes(n, P, n_dirs):
    """bytes of the caller-owned scratch of Handle.posterior_grad (fvgp_hip_posterior_grad_workspace_bytes); <= 0: invalid arguments"""
    return _workspace_bytes("fvgp_hip_posterior_grad_workspace_bytes", n, P, n_dirs)


def loo_workspace_bytes(n):
    """bytes of the caller-owned vector scratch of Handle.loo (fvgp_hip_loo_workspace_bytes); -1 for n < 1"""
    return _workspace_bytes("fvgp_hip_loo_workspace_bytes", n)


def mvn_sample_workspace_bytes(n, nsamp):
    """bytes of the caller-owned scratch of Handle.mvn_sample (fvgp_hip_mvn_sample_workspace_bytes); -1 for n < 1 or nsamp < 1"""
    return _workspace_bytes("fvgp_hip_mvn_sample_workspace_bytes", n, nsamp)


def select_workspace_bytes(n, P, q):
    """bytes of the caller-owned workspace of Handle.select_batch (fvgp_hip_select_workspace_bytes); -1 for n, P or q < 1"""
    return _workspace_bytes("fvgp_hip_select_workspace_bytes", n, P, q)


def kmatvec_workspace_bytes(n1, n2, s):
    """bytes of the split form's scratch of Handle.kmatvec (fvgp_hip_kmatvec_workspace_bytes); -1 for n1, n2 or s < 1"""
    return _workspace_bytes("fvgp_hip_kmatvec_workspace_bytes", n1, n2, s)


def pchol_workspace_bytes(n, q):
    """bytes of the caller-owned workspace of Handle.pchol (fvgp_hip_pchol_workspace_bytes); -1 for n or q < 1"""
    return _workspace_bytes("fvgp_hip_pchol_workspace_bytes", n, q)


def precond_workspace_bytes(n, q):
    """bytes of the caller-owned workspace of Handle.precond_factor (fvgp_hip_precond_workspace_bytes); -1 for n or q < 1"""
    return _workspace_bytes("fvgp_hip_precond_workspace_bytes", n, q)


def pcg_workspace_bytes(n, q):
    """bytes of the caller-owned workspace of Handle.pcg (fvgp_hip_pcg_workspace_bytes); -1 for n < 1 or q < 0"""
    return _workspace_bytes("fvgp_hip_pcg_workspace_bytes", n, q)


def pcg_lanczos_workspace_bytes(n, q, lanczos_steps):
    """bytes of the caller-owned workspace of Handle.pcg_lanczos (fvgp_hip_pcg_lanczos_workspace_bytes); -1 for bad arguments"""
    return _workspace_bytes("fvgp_hip_pcg_lanczos_workspace_bytes", n, q, lanczos_steps)


def kgrad_form_workspace_bytes(n1, n2):
    """bytes of the caller-owned workspace of Handle.kgrad_form (fvgp_hip_kgrad_form_workspace_bytes); -1 for n1 or n2 < 1"""
    return _workspace_bytes("fvgp_hip_kgrad_form_workspace_bytes", n1, n2)


def precond_apply_workspace_bytes(n, q):
    """bytes of the caller-owned workspace of Handle.precond_apply (fvgp_hip_precond_apply_workspace_bytes); -1 for n < 1 or q < 0"""
    return _workspace_bytes("fvgp_hip_precond_apply_workspace_bytes", n, q)


def chol_update_workspace_bytes(n, k):
    """bytes of the caller-owned workspace of Handle.chol_update / chol_delete (fvgp_hip_chol_update_workspace_bytes); -1 for n or k < 1"""
    return _workspace_bytes("fvgp_hip_chol_update_workspace_bytes", n, k)


def nn_workspace_bytes(what, nq, B=1):
    """bytes of the caller-owned workspace of Handle.nn_conditionals (what = NN_CONDITIONALS) / nn_loglik (NN_LOGLIK) for nq rows and B
    hyperparameter vectors (fvgp_hip_nn_workspace_bytes; NN_SEARCH takes none: 0); -1 for bad arguments"""
    return _workspace_bytes("fvgp_hip_nn_workspace_bytes", what, nq, B)


def nn_grad_workspace_bytes(n, B=1, ntheta=2):
    """bytes of the caller-owned workspace of Handle.nn_loglik_grad for n rows, B hyperparameter vectors of ntheta numbers
    (fvgp_hip_nn_grad_workspace_bytes); -1 for bad arguments"""
    return _workspace_bytes("fvgp_hip_nn_grad_workspace_bytes", n, B, ntheta)


def nn_fisher_workspace_bytes(n, B=1, ntheta=2):
    """bytes of the caller-owned workspace of Handle.nn_loglik_fisher for n rows, B hyperparameter vectors of ntheta numbers
    (fvgp_hip_nn_fisher_workspace_bytes); -1 for bad arguments"""
    return _workspace_bytes("fvgp_hip_nn_fisher_workspace_bytes", n, B, ntheta)


def nn_factor_workspace_bytes(n):
    """bytes of the caller-owned workspace of Handle.nn_factor for n rows (fvgp_hip_nn_factor_workspace_bytes); -1 for n < 1"""
    return _workspace_bytes("fvgp_hip_nn_factor_workspace_bytes", n)


def nn_precond_apply_workspace_bytes(n):
    """bytes of the caller-owned workspace of Handle.nn_precond_apply for n rows (fvgp_hip_nn_precond_apply_workspace_bytes); -1 for
    n < 1"""
    return _workspace_bytes("fvgp_hip_nn_precond_apply_workspace_bytes", n)


def pcg_nn_workspace_bytes(n):
    """bytes of the caller-owned workspace of Handle.pcg_nn for n rows (fvgp_hip_pcg_nn_workspace_bytes); -1 for n < 1"""
    return _workspace_bytes("fvgp_hip_pcg_nn_workspace_bytes", n)


def nn_transpose_lists(idx, n):
    """the transposed neighbour lists of idx (rows, ld) integers, on the host: (tr_start (n + 1,) int64, tr_pos (nnz,) int64).  Bucket j =
    tr_pos[tr_start[j]:tr_start[j + 1]] holds the flat positions i * ld + l of the entries with idx[i][l] == j in ascending i (and l):
    a stable argsort of the flattened lists, so the order -- and with it every sum over a bucket -- is the same on every call.  Entries
    outside 0 .. n - 1 belong to no bucket."""
    flat = np.ascontiguousarray(idx).reshape(-1).astype(np.int64)
    valid = (flat >= 0) & (flat < n)
    pos = np.flatnonzero(valid)
    order = np.argsort(flat[pos], kind="stable")
    start = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(flat[pos], minlength=n), out=start[1:])
    return start, pos[order].astype(np.int64)


class NNFactor:
    """The sparse inverse Cholesky factor W of Handle.nn_factor with its transposed lists, as Handle.nn_precond_apply and Handle.pcg_nn
    take it: device tensors idx (n, ld) int32, coef (n, ld), dinv (n), tr_start (n + 1) int64, tr_pos (max(nnz, 1)) int64, and m, nnz."""

    def __init__(self, idx, m, coef, dinv, tr_start, tr_pos, nnz):
        self.idx, self.m, self.coef, self.dinv, self.tr_start, self.tr_pos, self.nnz = idx, int(m), coef, dinv, tr_start, tr_pos, int(nnz)

    def _args(self):
        return (_ptr(self.idx), self.idx.stride(0), self.m, _ptr(self.coef), _ptr(self.dinv), _ptr(self.tr_start), _ptr(self.tr_pos), self.nnz)


def nn_maxmin_workspace_bytes(n):
    """bytes of the caller-owned workspace of Handle.nn_maxmin_order for n points (fvgp_hip_nn_maxmin_workspace_bytes); -1 for n < 1"""
    return _workspace_bytes("fvgp_hip_nn_maxmin_workspace_bytes", n)


def nn_grid_bytes(nr, d):
    """bytes of the device buffer that holds the cell grid of nr reference rows in d dimensions (fvgp_hip_nn_grid_bytes); -1 for
    nr < 1 or d outside 1 .. NN_GRID_MAX_DIM"""
    return _workspace_bytes("fvgp_hip_nn_grid_bytes", nr, d)


def nn_grid_workspace_bytes(nr, d):
    """bytes of the caller-owned workspace of Handle.nn_grid_build (fvgp_hip_nn_grid_workspace_bytes); -1 as nn_grid_bytes"""
    return _workspace_bytes("fvgp_hip_nn_grid_workspace_bytes", nr, d)


class NNGrid:
    """What Handle.nn_grid_build leaves for Handle.nn_grid_search: `buffer` (the device buffer with the bucketed rows), `info` (the host
    record, NN_GRID_INFO doubles) and the (nr, d) it was built over.  cells: the cells per dimension, edge: their scaled edge."""

    def __init__(self, buffer, info, nr, d):
        self.buffer, self.info, self.nr, self.d = buffer, info, int(nr), int(d)

    @property
    def cells(self):
        return tuple(int(c) for c in self.info[14:14 + self.d])

    @property
    def edge(self):
        return float(self.info[12])


def loglik_hess_workspace_bytes(n, d):
    """bytes of the caller-owned scratch of Handle.loglik_hess (fvgp_hip_loglik_hess_workspace_bytes); -1 for n < 1 or d outside 1..16"""
    return _workspace_bytes("fvgp_hip_loglik_hess_workspace_bytes", n, d)


def lib():
    """Load (once) and return the ctypes library with argtypes set."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HipExtensionError(
            f"{LIB_PATH} not found. The HIP extension is the product path and has no fallback; "
            f"build it with `python -c 'import __graft_entry__ as g; g.build()'` or `make -C {CSRC}`.")
    # torch first: libfvgp_hip.so must bind to the HIP runtime torch has loaded (its own copy), not bring /opt/rocm's in
    # beside it -- two runtimes in one process, and the one loaded first sees "no ROCm-capable device" once the other owns it
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    try:
        L = ctypes.CDLL(LIB_PATH)
    except OSError as e:
        raise HipExtensionError(f"cannot load {LIB_PATH}: {e}") from e
    missing = [s for s in SYMBOLS + SYMBOLS_NN if not hasattr(L, s)]
    if missing:
        raise HipExtensionError(f"{LIB_PATH} does not export {', '.join(missing)}: not a build of this ABI")
    _lib = bind(L)
    return _lib


def _check(rc, what):
    if rc != 0:
        msg = lib().fvgp_hip_last_error_string().decode(errors="replace")
        raise HipExtensionError(f"{what} failed with status {rc}" + (f": {msg}" if msg else ""))


def _theta(theta):
    t = np.ascontiguousarray(np.asarray(theta, dtype=np.float64))
    return t, t.ctypes.data_as(P_d), int(t.size)


def _ptr(t):
    """device pointer of a torch tensor (or None)."""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _scales_ptr(who, scales, d):
    """host pointer to the d scales of the nearest-neighbour binding `who`, or None (the pointer keeps its array alive)"""
    if scales is None:
        return None
    sc = np.ascontiguousarray(np.asarray(scales, dtype=np.float64))
    if sc.shape != (d,):
        raise ValueError(f"{who}: scales must be {d} numbers")
    return sc.ctypes.data_as(P_d)


def _batch_operands(who, x, thetas, vdiag, ymean):
    """the operands the batched entries share, as Handle method `who` passes them on: thetas as a contiguous (B, ntheta) array, vdiag as
    (1 or B, n) and ymean as (1 or B, n, ncol) with their per-problem strides in doubles (0 = one shared by every problem)"""
    t = np.ascontiguousarray(np.asarray(thetas, dtype=np.float64))
    if t.ndim != 2:
        raise ValueError(f"{who}: thetas must be (B, ntheta)")
    B, n = t.shape[0], x.shape[0]
    vd = vdiag.reshape(1, n) if vdiag.dim() == 1 else vdiag
    ym = ymean.reshape(1, *ymean.shape) if ymean.dim() == 2 else ymean
    for name, a in (("vdiag", vd), ("ymean", ym)):
        if a.shape[0] not in (1, B) or not a.is_contiguous():
            raise ValueError(f"{who}: {name} must be contiguous with a leading dimension of 1 or B = {B}, got {tuple(a.shape)}")
    return t, vd, n if vd.shape[0] > 1 else 0, ym, n * ym.shape[2] if ym.shape[0] > 1 else 0


def comm_unique_id():
    """128 bytes naming a new RCCL communicator (ncclGetUniqueId): rank 0 calls it and hands the bytes to every rank"""
    buf = ctypes.create_string_buffer(128)
    _check(lib().fvgp_hip_comm_unique_id(buf), "fvgp_hip_comm_unique_id")
    return bytes(buf.raw)


def create_stream(device, cu_mask=None, high_priority=False):
    """hipStream_t (as int) from fvgp_hip_stream_create: restricted to the CUs in `cu_mask` (iterable of CU
    indices) or an ordinary non-blocking stream."""
    out = ctypes.c_void_p()
    if cu_mask is None:
        _check(lib().fvgp_hip_stream_create(ctypes.byref(out), int(device), int(high_priority), None, 0), "fvgp_hip_stream_create")
    else:
        words = [0] * 8
        for cu in cu_mask:
            words[cu // 32] |= 1 << (cu % 32)
        arr = (ctypes.c_uint32 * 8)(*words)
        _check(lib().fvgp_hip_stream_create(ctypes.byref(out), int(device), 0, arr, 8), "fvgp_hip_stream_create")
    return out.value


def destroy_stream(stream):
    _check(lib().fvgp_hip_stream_destroy(ctypes.c_void_p(stream)), "fvgp_hip_stream_destroy")


class Handle(DistCalls):
    """One device + one stream.  Thin, argument-for-argument wrapper of the C ABI; tensors are
    torch CUDA fp64 tensors used purely as device-memory containers."""

    def __init__(self, device=0, stream=None):
        import torch
        if not torch.cuda.is_available():
            raise HipExtensionError("no HIP device visible (torch.cuda.is_available() is False); "
                                    "the native path has no CPU fallback")
        self.torch = torch
        self.device = int(device)
        self._h = ctypes.c_void_p()
        if stream is None:
            stream = torch.cuda.current_stream(self.device).cuda_stream
        _check(lib().fvgp_hip_create(ctypes.byref(self._h), self.device, ctypes.c_void_p(stream)), "fvgp_hip_create")
        for key in OPTION_KEYS:
            val = os.environ.get("FVGP_" + key.upper())
            if val is not None:
                self.set_option(key, int(val))

    def close(self):
        if self._h:
            lib().fvgp_hip_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- helpers -------------------------------------------------------------------------------
    def _call(self, name, *args):
        """the ABI entry `name` on this handle; a non-zero status raises"""
        _check(getattr(lib(), name)(self._h, *args), name)

    def _work(self, work, query, *sizes):
        """`work`, or for None a fresh device tensor of what the size query `query` asks for at `sizes` (none where it refuses them: the
        entry then names the bad argument)"""
        return self.empty(max(1, _workspace_bytes(query, *sizes)) // 8) if work is None else work

    def empty(self, *shape):
        return self.torch.empty(*shape, dtype=self.torch.float64, device=f"cuda:{self.device}")

    def zeros(self, *shape):
        return self.torch.zeros(*shape, dtype=self.torch.float64, device=f"cuda:{self.device}")

    def to_device(self, a):
        return self.torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=f"cuda:{self.device}")

    def to_host(self, t):
        """Device tensor (a strided view is fine) -> numpy array.  Results up to 1 GB (a posterior covariance at 1000 points is
        8 MB, at 4000 points 128 MB) come back through torch's cached PINNED host memory, which the returned array keeps alive:
        one DMA at the link's rate instead of a staged copy into freshly mapped pages (about 0.4 ms of 8.8 at N=20k, P=1000; 128 MB:
        3 ms instead of 15).  Anything larger takes the ordinary pageable path so that kept results cannot pin host memory
        without bound."""
        if t.numel() * t.element_size() > (1 << 30) or t.numel() == 0:
            return t.cpu().numpy()
        out = self.torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
        out.copy_(t, non_blocking=True)
        self.torch.cuda.current_stream(self.device).synchronize()
        return out.numpy()

    def sync(self):
        self._call("fvgp_hip_sync")

    def set_option(self, key, value):
        self._call("fvgp_hip_set_option", key.encode(), int(value))

    def invalidate_factor(self):
        """Forget the cached diagonal-block inverses: call after writing a factor buffer by anything but potrf."""
        self._call("fvgp_hip_invalidate_factor")

    def get_profile(self):
        out = (ctypes.c_double * 16)()
        self._call("fvgp_hip_get_profile_ex", out)
        return {"launches": out[0], "ms": out[1], "flops": out[2], "potrf_ms": out[3],
                "kmat_ms": out[4], "kmat_bytes": out[5], "tail_ms": out[6], "host_enqueue_ms": out[7], "bytes": out[8]}

    def chain_verify_counts(self):
        """(mismatches, comparisons) of the resident panel kernel's hand-off checksums since the last call (option "chain_verify")"""
        out = (ctypes.c_int64 * 2)()
        self._call("fvgp_hip_chain_verify_counts", out)
        return int(out[0]), int(out[1])

    # -- ABI calls -----------------------------------------------------------------------------
    def kmat(self, kernel_id, x1, x2, theta, K, vdiag=None, uplo=FULL, pad=PAD_NONE):
        t, tp, nt = _theta(theta)
        self._call("fvgp_hip_kmat", int(kernel_id), _ptr(x1), x1.shape[0], _ptr(x2), x2.shape[0],
                   x1.shape[1], tp, nt, _ptr(vdiag), _ptr(K), K.stride(0), int(uplo), int(pad))

    def potrf(self, A, n):
        info = ctypes.c_int(0)
        self._call("fvgp_hip_potrf", _ptr(A), int(n), A.stride(0), ctypes.byref(info))
        return info.value

    def potrs(self, L, n, B, nrhs):
        self._call("fvgp_hip_potrs", _ptr(L), int(n), L.stride(0), _ptr(B), int(nrhs), B.stride(0))

    def trsm_lower(self, L, n, B, nrhs):
        self._call("fvgp_hip_trsm_lower", _ptr(L), int(n), L.stride(0), _ptr(B), int(nrhs), B.stride(0))

    def trsm_lower_t(self, L, n, B, nrhs):
        self._call("fvgp_hip_trsm_lower_t", _ptr(L), int(n), L.stride(0), _ptr(B), int(nrhs), B.stride(0))

    def panel_trsm(self, D, nd, P, rows):
        self._call("fvgp_hip_panel_trsm", _ptr(D), int(nd), D.stride(0), _ptr(P), int(rows), P.stride(0))

    def syrk_rowshard(self, M, N, K, A, B, C, scale, off, b_ranks=1, b_blocks=0, b_off=0):
        self._call("fvgp_hip_syrk_rowshard", int(M), int(N), int(K), _ptr(A), A.stride(0), _ptr(B), B.stride(0),
                   _ptr(C), C.stride(0), int(scale), int(off), int(b_ranks), int(b_blocks), int(b_off))

    def panel_potrf_dev(self, T, w, rows, n_valid, info_dev, logdet_dev):
        """Enqueue-only factorisation of a tall panel (diagonal block on top, this rank's rows below)."""
        self._call("fvgp_hip_panel_potrf_dev", _ptr(T), int(w), int(rows), T.stride(0), int(n_valid), _ptr(info_dev),
                   _ptr(logdet_dev) if logdet_dev is not None else None)

    def potrf_dev(self, A, n, n_logdet, info_dev, logdet_dev):
        """Enqueue-only potrf: info (int32 tensor) and log-det (float64 tensor) stay on the device."""
        self._call("fvgp_hip_potrf_dev", _ptr(A), int(n), A.stride(0), int(n_logdet), _ptr(info_dev),
                   _ptr(logdet_dev) if logdet_dev is not None else None)

    def logdet(self, L, n):
        out = ctypes.c_double(0.0)
        self._call("fvgp_hip_logdet", _ptr(L), int(n), L.stride(0), ctypes.byref(out))
        return out.value

    def potri(self, L, n, work):
        self._call("fvgp_hip_potri", _ptr(L), int(n), L.stride(0), _ptr(work), work.stride(0))

    def loglik(self, kernel_id, x, theta, vdiag, ymean, KV, alpha):
        """fvgp_hip_loglik_rows: the scratch's ROWS are passed as the tensor has them (KV.shape[0]), never inferred from its stride --
        the forward solve is fused for every n when KV is a square of loglik_dim(n, ncol)"""
        t, tp, nt = _theta(theta)
        out = (ctypes.c_double * 3)()
        info = ctypes.c_int(0)
        n, d = x.shape
        if KV.dim() != 2 or KV.stride(1) != 1 or KV.shape[1] < pad128(n) or KV.shape[0] < pad128(n):
            raise ValueError(f"loglik: KV must be a row-major 2-d tensor of at least {pad128(n)} x {pad128(n)}, got {tuple(KV.shape)} strides {KV.stride()}")
        # the extra block row is only claimed when the tensor owns those rows AND columns (a column slice with a wide stride does not)
        rows = KV.shape[0] if KV.shape[1] >= loglik_dim(n, ymean.shape[1]) else pad128(n)
        self._call("fvgp_hip_loglik_rows", int(kernel_id), _ptr(x), n, d, tp, nt, _ptr(vdiag), _ptr(ymean),
                   ymean.shape[1], _ptr(KV), rows, KV.stride(0), _ptr(alpha), out, ctypes.byref(info))
        return out[0], out[1], out[2], info.value

    def loglik_batch(self, kernel_id, x, thetas, vdiag, ymean, KV):
        """fvgp_hip_loglik_batch: the log marginal likelihood at the B rows of `thetas` (host, B x ntheta) in one call.
        vdiag (1, n) / ymean (1, n, ncol) -- or 1-d / 2-d -- are shared by every problem; (B, n) / (B, n, ncol) give each its own.
        KV: (B, dim, ld) device scratch, dim = loglik_batch_dim(n, ncol) (or any tensor whose first dimension strides the squares).
        Returns (out (B, 3) ndarray of {log-likelihood, log|KV|, quad / ncol}, NaN where the factorisation failed; info (B,) ints)."""
        t, vd, vd_stride, ym, ym_stride = _batch_operands("loglik_batch", x, thetas, vdiag, ymean)
        (B, nt), (n, d), ncol = t.shape, x.shape, ym.shape[2]
        if KV.dim() != 3 or KV.stride(2) != 1 or (B > 1 and KV.shape[0] < B):
            raise ValueError(f"loglik_batch: KV must be a (B, dim, ld) tensor with unit column stride, got {tuple(KV.shape)}")
        out = np.empty((B, 3), dtype=np.float64)
        info = np.zeros(B, dtype=np.int32)
        self._call("fvgp_hip_loglik_batch", int(kernel_id), _ptr(x), n, d, t.ctypes.data_as(P_d), nt, B,
                   _ptr(vd), vd_stride, _ptr(ym), ym_stride, ncol,
                   _ptr(KV), KV.stride(1), KV.stride(0), out.ctypes.data_as(P_d), info.ctypes.data_as(P_i))
        return out, info

    def loglik_grad_batch(self, kernel_id, x, thetas, vdiag, ymean, KV, work, component=0, b_out=None, diag_out=None):
        """fvgp_hip_loglik_grad_batch: loglik_batch's values and the kernel-owned gradient at the B rows of `thetas` in one call.
        vdiag / ymean / KV as loglik_batch; work: (B, rows, ldw) second device scratch, rows >= pad128(n).  b_out / diag_out: optional
        (B, n) device tensors for b = KV^-1 (y - m)[:, component] and diag(KV^-1).  Returns (out (B, 3), grad (B, ntheta), info (B,)):
        NaN rows where the factorisation failed."""
        t, vd, vd_stride, ym, ym_stride = _batch_operands("loglik_grad_batch", x, thetas, vdiag, ymean)
        (B, nt), (n, d), ncol = t.shape, x.shape, ym.shape[2]
        for name, a in (("KV", KV), ("work", work)):
            if a.dim() != 3 or a.stride(2) != 1 or (B > 1 and a.shape[0] < B):
                raise ValueError(f"loglik_grad_batch: {name} must be a (B, rows, ld) tensor with unit column stride, got {tuple(a.shape)}")
        for name, a in (("b_out", b_out), ("diag_out", diag_out)):
            if a is not None and (not a.is_contiguous() or a.numel() < B * n):
                raise ValueError(f"loglik_grad_batch: {name} must be a contiguous (B, n) tensor, got {tuple(a.shape)}")
        out = np.empty((B, 3), dtype=np.float64)
        grad = np.empty((B, nt), dtype=np.float64)
        info = np.zeros(B, dtype=np.int32)
        self._call("fvgp_hip_loglik_grad_batch", int(kernel_id), _ptr(x), n, d, t.ctypes.data_as(P_d), nt, B,
                   _ptr(vd), vd_stride, _ptr(ym), ym_stride, ncol,
                   int(component), _ptr(KV), KV.stride(1), KV.stride(0), _ptr(work), work.stride(1), work.stride(0),
                   out.ctypes.data_as(P_d), grad.ctypes.data_as(P_d), info.ctypes.data_as(P_i),
                   _ptr(b_out), _ptr(diag_out))
        return out, grad, info

    def posterior_batch(self, kernel_id, x, thetas, vdiag, ymean, xpred, KV, mean_out, var_out=None, S_out=None, want_loglik=False):
        """fvgp_hip_posterior_batch: posterior mean, variance and covariance at the B rows of `thetas` (host, B x ntheta) and the P rows
        of `xpred` (device, P x d) in one call.  vdiag / ymean as loglik_batch.  KV: (B, loglik_batch_dim(n, ncol) + P_chunk, ld) device
        scratch, P_chunk (a multiple of 128) the prediction points per pass; mean_out (B, P, ncol), var_out (B, P) or None, S_out
        (B, >= pad128(P), lds) or None: device tensors that receive V^T z (no prior mean), the unclipped variance and the full symmetric
        covariance (S_out needs P <= P_chunk).  Returns (out, info): out the (B, 3) array loglik_batch returns (None unless want_loglik),
        info (B,) ints; rows with info > 0 hold NaN."""
        t, vd, vd_stride, ym, ym_stride = _batch_operands("posterior_batch", x, thetas, vdiag, ymean)
        (B, nt), (n, d), ncol = t.shape, x.shape, ym.shape[2]
        if xpred.dim() != 2 or xpred.shape[1] != d or not xpred.is_contiguous():
            raise ValueError(f"posterior_batch: xpred must be a contiguous (P, {d}) tensor, got {tuple(xpred.shape)}")
        P = xpred.shape[0]
        if KV.dim() != 3 or KV.stride(2) != 1 or (B > 1 and KV.shape[0] < B):
            raise ValueError(f"posterior_batch: KV must be a (B, rows, ld) tensor with unit column stride, got {tuple(KV.shape)}")
        if not mean_out.is_contiguous() or mean_out.numel() < B * P * ncol:
            raise ValueError(f"posterior_batch: mean_out must be a contiguous (B, P, ncol) tensor, got {tuple(mean_out.shape)}")
        if var_out is not None and (not var_out.is_contiguous() or var_out.numel() < B * P):
            raise ValueError(f"posterior_batch: var_out must be a contiguous (B, P) tensor, got {tuple(var_out.shape)}")
        if S_out is not None and (S_out.dim() != 3 or S_out.stride(2) != 1 or S_out.shape[1] < pad128(P) or (B > 1 and S_out.shape[0] < B)):
            raise ValueError(f"posterior_batch: S_out must be a (B, >= {pad128(P)}, lds) tensor with unit column stride, got {tuple(S_out.shape)}")
        out = np.empty((B, 3), dtype=np.float64) if want_loglik else None
        info = np.zeros(B, dtype=np.int32)
        self._call("fvgp_hip_posterior_batch", int(kernel_id), _ptr(x), n, d, t.ctypes.data_as(P_d), nt, B,
                   _ptr(vd), vd_stride, _ptr(ym), ym_stride, ncol,
                   _ptr(xpred), P, _ptr(KV), KV.shape[1], KV.stride(1), KV.stride(0),
                   _ptr(mean_out), _ptr(var_out), _ptr(S_out),
                   0 if S_out is None else S_out.stride(1), 0 if S_out is None else S_out.stride(0),
                   None if out is None else out.ctypes.data_as(P_d), info.ctypes.data_as(P_i))
        return out, info

    def loglik_grad(self, kernel_id, x, theta, alpha, ncol, component, KV, work):
        t, tp, nt = _theta(theta)
        g = (ctypes.c_double * nt)()
        n, d = x.shape
        self._call("fvgp_hip_loglik_grad", int(kernel_id), _ptr(x), n, d, tp, nt, _ptr(alpha), int(ncol),
                   int(component), _ptr(KV), KV.stride(0), _ptr(work), work.stride(0), g)
        return np.array(g[:], dtype=np.float64)

    def loglik_hess(self, kernel_id, x, theta, alpha, ncol, component, KV, work, work2, ws):
        """fvgp_hip_loglik_hess on the factor in KV (destroyed, as `work` and `work2`, two more padded squares): returns (grad, raw)
        with grad the kernel-owned gradient of the negative log-likelihood (the rest 0) and raw the (nk, nk) Hessian block as the
        device computed it, row i from G_i = W K_i W -- NOT symmetrised.  ws: a tensor of at least loglik_hess_workspace_bytes(n, d)
        bytes.  One synchronisation."""
        t, tp, nt = _theta(theta)
        n, d = x.shape
        nk = 2 if int(kernel_id) in _ISO_IDS else d + 1
        g = (ctypes.c_double * nt)()
        hs = (ctypes.c_double * (nk * nk))()
        self._call("fvgp_hip_loglik_hess", int(kernel_id), _ptr(x), n, d, tp, nt, _ptr(alpha), int(ncol), int(component),
                   _ptr(KV), KV.stride(0), _ptr(work), work.stride(0), _ptr(work2), work2.stride(0),
                   _ptr(ws), ws.numel() * ws.element_size(), g, hs)
        return np.array(g[:], dtype=np.float64), np.array(hs[:], dtype=np.float64).reshape(nk, nk)

    def grad_trace(self, kernel_id, x, theta, W, b, partial):
        """1/2 sum_jk (W_jk - b_j b_k) dK_jk/dtheta_i over the symmetric W (lower triangle read); b a 1-d view or None.
        W: 16-byte aligned with an even row stride >= pad128(n) (status -9 otherwise): the pass loads whole 128-column tile rows.
        partial: device scratch of T (T + 1) / 2 * ntheta doubles, T = ceil(n / 128)."""
        t, tp, nt = _theta(theta)
        g = (ctypes.c_double * nt)()
        n, d = x.shape
        self._call("fvgp_hip_grad_trace", int(kernel_id), _ptr(x), n, d, tp, nt, _ptr(W), W.stride(0),
                   _ptr(b), 1 if b is None else b.stride(0), _ptr(partial), g)
        return np.array(g[:], dtype=np.float64)

    def grad_trace_cols(self, kernel_id, x, theta, W, col0, ncols, b, partial):
        """the same pass over the slab W (n, >= pad128(ncols)) of columns [col0, col0 + ncols) of the symmetric matrix (col0 % 128 == 0;
        a row stride below pad128(ncols): status -9); partial: ceil(n / 128) * ceil(ncols / 128) * ntheta doubles"""
        t, tp, nt = _theta(theta)
        g = (ctypes.c_double * nt)()
        n, d = x.shape
        self._call("fvgp_hip_grad_trace_cols", int(kernel_id), _ptr(x), n, d, tp, nt, _ptr(W), W.stride(0), int(col0), int(ncols),
                   _ptr(b), 1 if b is None else b.stride(0), _ptr(partial), g)
        return np.array(g[:], dtype=np.float64)

    # -- row-sharded evaluation (include/fvgp_hip.h: fvgp_hip_comm_* / fvgp_hip_loglik_dist) ---------------------------
    def comm_init(self, unique_id, rank, nranks):
        """bind RCCL: unique_id = the 128 bytes of comm_unique_id() on rank 0, handed to every rank by the caller"""
        buf = ctypes.create_string_buffer(bytes(unique_id), 128)
        self._call("fvgp_hip_comm_init", buf, int(rank), int(nranks))

    def comm_init_callbacks(self, coll, rank, nranks):
        self._coll = coll                                          # the callbacks must outlive the handle's use of them
        self._call("fvgp_hip_comm_init_callbacks", ctypes.byref(coll), int(rank), int(nranks))

    def ipc_window(self, window_bytes):
        """allocate this rank's window of the direct (IPC) collectives; returns its 64-byte handle"""
        buf = ctypes.create_string_buffer(64)
        self._call("fvgp_hip_ipc_window", int(window_bytes), buf)
        return buf.raw

    def comm_init_ipc(self, all_handles, shm_name, rank, nranks):
        """bind the direct collectives: all_handles = the ranks' 64-byte window handles in rank order"""
        blob = ctypes.create_string_buffer(b"".join(bytes(hd) for hd in all_handles), 64 * int(nranks))
        self._call("fvgp_hip_comm_init_ipc", blob, shm_name.encode(), int(rank), int(nranks))

    def comm_destroy(self):
        self._call("fvgp_hip_comm_destroy")

    def all_reduce(self, t):
        self._call("fvgp_hip_all_reduce", _ptr(t), t.numel())

    def all_gather(self, send, recv):
        self._call("fvgp_hip_all_gather", _ptr(send), _ptr(recv), send.numel())

    def _dist_lib(self):
        return lib()

    @staticmethod
    def _dist_check(rc, what):
        _check(rc, what)

    def comm_info(self):
        """the handle's communicator as it reports itself (fvgp_hip_comm_info)"""
        out = (ctypes.c_int64 * 8)()
        self._call("fvgp_hip_comm_info", out)
        info = {"kind": {0: "none", 1: "rccl", 2: "ipc", 3: "callbacks"}[int(out[0])], "nranks_bound": int(out[1]), "rank_bound": int(out[2])}
        if out[0] == 1:
            info.update(nccl_comm_count=int(out[3]), nccl_comm_user_rank=int(out[4]), nccl_comm_cu_device=int(out[5]), rccl_version=int(out[6]))
        return info

    def comm_check(self):
        self._call("fvgp_hip_comm_check")

    def comm_profile(self):
        out = (ctypes.c_double * 6)()
        self._call("fvgp_hip_comm_profile", out)
        return {"all_gather": (int(out[0]), out[2], out[4]), "all_reduce": (int(out[1]), out[3], out[5])}

    def dist_workspace(self, desc):
        out = (ctypes.c_int64 * 6)()
        _check(lib().fvgp_hip_dist_workspace(ctypes.byref(desc), out), "fvgp_hip_dist_workspace")
        return list(out)

    def loglik_dist(self, desc, theta):
        t, tp, nt = _theta(theta)
        out = (ctypes.c_double * 3)()
        info = ctypes.c_int(0)
        self._call("fvgp_hip_loglik_dist", ctypes.byref(desc), tp, nt, out, ctypes.byref(info))
        return out[0], out[1], out[2], info.value

    def posterior(self, kernel_id, x, theta, L, alpha, ncol, xpred, kx, mean_out=None, var_out=None, S_out=None):
        t, tp, nt = _theta(theta)
        n, d = x.shape
        self._call("fvgp_hip_posterior", int(kernel_id), _ptr(x), n, d, tp, nt, _ptr(L), L.stride(0),
                   _ptr(alpha), int(ncol), _ptr(xpred), xpred.shape[0], _ptr(kx), kx.stride(0),
                   _ptr(mean_out), _ptr(var_out), _ptr(S_out), 0 if S_out is None else S_out.stride(0))

    def posterior_grad(self, kernel_id, x, theta, xpred, alpha, ncol, component, W, n_dirs, work, A_out, q_out, dm_out, dv_out):
        """fvgp_hip_posterior_grad: A = k^T alpha[:, component], q = sum_i k_i W_i and their exact derivatives dm, dv (P, n_dirs) in the
        first n_dirs columns of the prediction points; W = KV^-1 k(x, xpred) (padded n x >= padded P) or None for the mean only;
        work: a tensor of at least posterior_grad_workspace_bytes(n, P, n_dirs) bytes.  Asynchronous."""
        t, tp, nt = _theta(theta)
        n, d = x.shape
        self._call("fvgp_hip_posterior_grad", int(kernel_id), _ptr(x), n, d, tp, nt, _ptr(xpred), xpred.shape[0],
                   _ptr(alpha), int(ncol), int(component), _ptr(W), 0 if W is None else W.stride(0),
                   int(n_dirs), _ptr(work), work.numel() * work.element_size(),
                   _ptr(A_out), _ptr(q_out), _ptr(dm_out), _ptr(dv_out))

    def loo(self, kernel_id, x, theta, alpha, ncol, component, KV, work, ws, resid_out, var_out, u_out=None, mdiag_out=None, n=None):
        """fvgp_hip_loo on the factor in KV (destroyed, as `work`): returns (out, grad) with out = [L_LOO, sum resid^2, sum log q_i,
        number of q_i that are not positive and finite] and grad = dL_LOO/dtheta (kernel-owned entries, the rest 0).  u_out and
        mdiag_out None: values only, grad is None and kernel_id, x, theta may be None (pass n then).  ws: a tensor of at least
        loo_workspace_bytes(n) bytes; resid_out, var_out, u_out, mdiag_out: device n-vectors.  One synchronisation."""
        want_grad = u_out is not None or mdiag_out is not None
        if want_grad:
            t, tp, nt = _theta(theta)
            g = (ctypes.c_double * nt)()
            n, d = x.shape
        else:
            tp, nt, g, d = None, 0, None, 0 if x is None else x.shape[1]
            n = int(x.shape[0] if n is None else n)
        out = (ctypes.c_double * 4)()
        self._call("fvgp_hip_loo", int(kernel_id or 0), _ptr(x), n, d, tp, nt, _ptr(alpha), int(ncol), int(component),
                   _ptr(KV), KV.stride(0), _ptr(work), work.stride(0), _ptr(ws), ws.numel() * ws.element_size(),
                   out, _ptr(resid_out), _ptr(var_out), g, _ptr(u_out), _ptr(mdiag_out))
        return np.array(out[:], dtype=np.float64), (None if g is None else np.array(g[:], dtype=np.float64))

    def normal_fill(self, Z, seed=0, stream=0, row0=0, col0=0):
        """fvgp_hip_normal_fill: Z[r][c] = z(seed, stream, row0 + r, col0 + c) over the whole 2-d device tensor Z (a view with a
        larger row stride is fine: only its rows x cols entries are written).  Asynchronous."""
        assert Z.dim() == 2 and Z.stride(1) == 1, "Z must be a 2-d tensor with contiguous rows"
        self._call("fvgp_hip_normal_fill", int(seed), int(stream), int(row0), int(col0), _ptr(Z), Z.shape[0], Z.shape[1], Z.stride(0))

    def mvn_sample(self, L, n, Y, mean=None, seed=0, stream=0, samp0=0, Z_out=None, work=None):
        """fvgp_hip_mvn_sample: Y[s] = mean + tril(L) z(seed, stream, :, samp0 + s) for the Y.shape[0] rows of the device tensor Y
        (nsamp, >= n); L the padded factor of an n x n matrix, mean a device n-vector or None, Z_out None or a device (n, >= nsamp)
        tensor that receives the normals, work None (allocated here) or a flat device tensor of mvn_sample_workspace_bytes(n, nsamp)
        bytes.  Asynchronous; a sample's bits depend on (seed, stream, its index) and L only."""
        nsamp = int(Y.shape[0])
        work = self._work(work, "fvgp_hip_mvn_sample_workspace_bytes", n, nsamp)
        self._call("fvgp_hip_mvn_sample", _ptr(L), int(n), L.stride(0), _ptr(mean), int(seed), int(stream), int(samp0), nsamp,
                   _ptr(Y), Y.stride(0), _ptr(Z_out), 0 if Z_out is None else Z_out.stride(0),
                   _ptr(work), work.numel() * 8)

    def select_batch(self, kernel_id, x, theta, L, xcand, var, q, idx_out, pick_var_out, noise=None, criterion=0, allow_repeats=False,
                     tol=1e-12, G_out=None, work=None):
        """fvgp_hip_select_batch: the greedy batch of q of the xcand.shape[0] candidates on the factor L of K + V over x.  var (P): in
        the candidates' posterior variances, out their variances after the batch; noise (P) device vector or None (= 0); idx_out an
        int64 device (q,) tensor (-1 from the first exhausted step on), pick_var_out (q); G_out None or a device (q, >= P) tensor;
        criterion 0 = variance, 1 = information (needs noise > 0); work None (allocated here) or a flat device tensor of
        select_workspace_bytes(n, P, q) bytes.  Asynchronous."""
        t, tp, nt = _theta(theta)
        n, d = x.shape
        P = int(xcand.shape[0])
        work = self._work(work, "fvgp_hip_select_workspace_bytes", n, P, q)
        self._call("fvgp_hip_select_batch", int(kernel_id), _ptr(x), n, d, tp, nt, _ptr(L), L.stride(0), _ptr(xcand), P,
                   _ptr(noise), _ptr(var), int(q), int(criterion), int(bool(allow_repeats)), float(tol),
                   _ptr(work), work.numel() * 8, _ptr(idx_out), _ptr(pick_var_out), _ptr(G_out),
                   0 if G_out is None else G_out.stride(0))

    def kmatvec(self, kernel_id, x1, x2, theta, B, Y, vdiag=None, s=None, work=None):
        """fvgp_hip_kmatvec: Y[:, :s] = K(x1, x2) B[:, :s] + diag(vdiag) B[:, :s] without K.  B (n2, >= s), Y (n1, >= s) device
        tensors (strided views are fine), vdiag (n1) or None (needs n1 == n2); work None or a flat device tensor for the split form
        (kmatvec_workspace_bytes).  Asynchronous."""
        t, tp, nt = _theta(theta)
        s = int(B.shape[1] if s is None else s)
        self._call("fvgp_hip_kmatvec", int(kernel_id), _ptr(x1), x1.shape[0], _ptr(x2), x2.shape[0], x1.shape[1], tp, nt,
                   _ptr(vdiag), _ptr(B), B.stride(0), s, _ptr(Y), Y.stride(0), _ptr(work),
                   0 if work is None else work.numel() * 8)

    def pchol(self, kernel_id, x, theta, q, G, piv_out, tol=0.0, resid_diag_out=None, work=None):
        """fvgp_hip_pchol: the greedy pivoted Cholesky of K(x, x), rank <= q, into G (q, >= n); piv_out an int64 device (q,) tensor
        (-1 from the achieved rank on, the rows of G there are zero); returns the achieved rank (synchronises)."""
        t, tp, nt = _theta(theta)
        n, d = x.shape
        work = self._work(work, "fvgp_hip_pchol_workspace_bytes", n, q)
        rank = ctypes.c_int(0)
        self._call("fvgp_hip_pchol", int(kernel_id), _ptr(x), n, d, tp, nt, int(q), float(tol), _ptr(G), G.stride(0),
                   _ptr(piv_out), _ptr(resid_diag_out), _ptr(work), work.numel() * 8, ctypes.byref(rank))
        return int(rank.value)

    def precond_factor(self, G, q, n, vdiag, C, work=None):
        """fvgp_hip_precond_factor: C (padded_dim(q) square) <- the factor of I + G D^-1 G^T; returns info (0 = factored)"""
        work = self._work(work, "fvgp_hip_precond_workspace_bytes", n, q)
        info = ctypes.c_int(0)
        self._call("fvgp_hip_precond_factor", _ptr(G), G.stride(0), int(q), int(n), _ptr(vdiag), _ptr(C), C.stride(0),
                   _ptr(work), work.numel() * 8, ctypes.byref(info))
        return int(info.value)

    def pcg(self, kernel_id, x, theta, vdiag, B, X, G=None, q=0, C=None, s=None, warm=False, tol=1e-10, max_iter=1000, check_every=8,
            max_restarts=3, work=None):
        """fvgp_hip_pcg: (K(x, x) + diag(vdiag)) X[:, :s] = B[:, :s], s <= PCG_MAX_RHS, preconditioned by (G, C) of pchol /
        precond_factor (G None or q == 0: Jacobi).  Returns (iters, relres, status) as numpy arrays of s entries: status 0 converged,
        1 not converged, 2 breakdown; relres is the true relative residual.  Synchronous."""
        t, tp, nt = _theta(theta)
        n, d = x.shape
        s = int(B.shape[1] if s is None else s)
        q = 0 if G is None else int(q)
        work = self._work(work, "fvgp_hip_pcg_workspace_bytes", n, q)
        iters = np.zeros(max(s, 1), dtype=np.int32)
        status = np.zeros(max(s, 1), dtype=np.int32)
        relres = np.zeros(max(s, 1), dtype=np.float64)
        self._call("fvgp_hip_pcg", int(kernel_id), _ptr(x), n, d, tp, nt, _ptr(vdiag), _ptr(G),
                   0 if G is None else G.stride(0), q, _ptr(C), 0 if C is None else C.stride(0),
                   _ptr(B), B.stride(0), s, _ptr(X), X.stride(0), int(bool(warm)), float(tol), int(max_iter),
                   int(check_every), int(max_restarts), _ptr(work), work.numel() * 8,
                   iters.ctypes.data_as(P_i), relres.ctypes.data_as(P_d), status.ctypes.data_as(P_i))
        return iters[:s], relres[:s], status[:s]

    def pcg_lanczos(self, kernel_id, x, theta, vdiag, B, X, lanczos_steps, G=None, q=0, C=None, s=None, warm=False, tol=1e-10,
                    max_iter=1000, check_every=8, max_restarts=3, work=None):
        """fvgp_hip_pcg_lanczos: Handle.pcg that also records the coefficients of every column's first recurrence.  Returns (iters,
        relres, status, alpha (s, L), beta (s, L), steps (s), rho0 (s)); with lanczos_steps == 0 the last four are empty."""
        t, tp, nt = _theta(theta)
        n, d = x.shape
        s = int(B.shape[1] if s is None else s)
        q = 0 if G is None else int(q)
        L = int(lanczos_steps)
        work = self._work(work, "fvgp_hip_pcg_lanczos_workspace_bytes", n, q, L)
        iters = np.zeros(max(s, 1), dtype=np.int32)
        status = np.zeros(max(s, 1), dtype=np.int32)
        relres = np.zeros(max(s, 1), dtype=np.float64)
        alpha, beta = np.zeros((max(s, 1), max(L, 1))), np.zeros((max(s, 1), max(L, 1)))
        steps, rho0 = np.zeros(max(s, 1), dtype=np.int32), np.zeros(max(s, 1))
        self._call("fvgp_hip_pcg_lanczos", int(kernel_id), _ptr(x), n, d, tp, nt, _ptr(vdiag), _ptr(G),
                   0 if G is None else G.stride(0), q, _ptr(C), 0 if C is None else C.stride(0),
                   _ptr(B), B.stride(0), s, _ptr(X), X.stride(0), int(bool(warm)), float(tol), int(max_iter),
                   int(check_every), int(max_restarts), _ptr(work), work.numel() * 8,
                   iters.ctypes.data_as(P_i), relres.ctypes.data_as(P_d), status.ctypes.data_as(P_i), L,
                   alpha.ctypes.data_as(P_d), beta.ctypes.data_as(P_d), steps.ctypes.data_as(P_i),
                   rho0.ctypes.data_as(P_d))
        if L == 0:
            return iters[:s], relres[:s], status[:s], alpha[:s, :0], beta[:s, :0], steps[:0], rho0[:0]
        return iters[:s], relres[:s], status[:s], alpha[:s], beta[:s], steps[:s], rho0[:s]

    def kgrad_form(self, kernel_id, x1, U, x2, W, theta, s=None, work=None):
        """fvgp_hip_kgrad_form: the vector of sum_{c < s} U[:, c]^T (dK(x1, x2) / dtheta_j) W[:, c] over the kernel's own hyperparameters
        (sigma^2, then the length scales), K never formed.  U (n1, >= s), W (n2, >= s) device tensors; synchronous."""
        t, tp, nt = _theta(theta)
        s = int(U.shape[1] if s is None else s)
        n1, n2 = x1.shape[0], x2.shape[0]
        work = self._work(work, "fvgp_hip_kgrad_form_workspace_bytes", n1, n2)
        out = np.zeros(max(nt, 1), dtype=np.float64)
        self._call("fvgp_hip_kgrad_form", int(kernel_id), _ptr(x1), n1, _ptr(x2), n2, x1.shape[1], tp, nt, _ptr(U), U.stride(0),
                   _ptr(W), W.stride(0), s, _ptr(work), work.numel() * 8, out.ctypes.data_as(P_d))
        return out

    def precond_probes(self, Z, vdiag, G=None, q=0, seed=0, stream=0, col0=0):
        """fvgp_hip_precond_probes: Z[:, c] = D^1/2 z(seed, 2 stream, :, col0 + c) + G^T z(seed, 2 stream + 1, :, col0 + c) over the
        columns of the device tensor Z (n, s <= PCG_MAX_RHS): probes with covariance G^T G + D.  Asynchronous."""
        q = 0 if G is None else int(q)
        self._call("fvgp_hip_precond_probes", int(seed), int(stream), int(col0), _ptr(G), 0 if G is None else G.stride(0), q,
                   Z.shape[0], _ptr(vdiag), _ptr(Z), Z.stride(0), Z.shape[1])

    def precond_apply(self, R, W, vdiag, G=None, q=0, C=None, s=None, work=None):
        """fvgp_hip_precond_apply: W[:, :s] = (G^T G + D)^-1 R[:, :s] with the factor C of precond_factor (G None: D^-1 R), by the
        solver's own launches.  Asynchronous."""
        n = R.shape[0]
        s = int(R.shape[1] if s is None else s)
        q = 0 if G is None else int(q)
        work = self._work(work, "fvgp_hip_precond_apply_workspace_bytes", n, q)
        self._call("fvgp_hip_precond_apply", _ptr(G), 0 if G is None else G.stride(0), q, _ptr(C),
                   0 if C is None else C.stride(0), n, _ptr(vdiag), _ptr(R), R.stride(0), s, _ptr(W),
                   W.stride(0), _ptr(work), work.numel() * 8)

    def potrs_cols(self, L, n, B, nrhs):
        """Handle.potrs for nrhs % 128 == 0 columns whose bits do not depend on nrhs (fvgp_hip_potrs_cols)"""
        self._call("fvgp_hip_potrs_cols", _ptr(L), n, L.stride(0), _ptr(B), nrhs, B.stride(0))

    def chol_update(self, L, n, W, k=None, row0=0, work=None):
        """fvgp_hip_chol_update: L <- chol(L L^T + W[:, :k] W[:, :k]^T) in place on the n leading rows; W (n, >= k) device, destroyed, its
        rows < row0 zero.  Asynchronous; call invalidate_factor() before the next solve with L."""
        k = int(W.shape[1] if k is None else k)
        if work is None:
            work = self.empty(CHOL_UPDATE_TABLE_BYTES // 8)
        self._call("fvgp_hip_chol_update", _ptr(L), int(n), L.stride(0), _ptr(W), k, W.stride(0), int(row0), _ptr(work), work.numel() * 8)

    def chol_delete(self, L, n, idx, work=None):
        """fvgp_hip_chol_delete: the factor of the points that remain when the strictly increasing indices `idx` (host) leave, in the same
        buffer and as potrf leaves a factor of n - len(idx) points.  Asynchronous; call invalidate_factor() before the next solve."""
        idx = np.ascontiguousarray(np.asarray(idx, dtype=np.int64).ravel())
        work = self._work(work, "fvgp_hip_chol_update_workspace_bytes", n, len(idx))
        self._call("fvgp_hip_chol_delete", _ptr(L), int(n), L.stride(0), idx.ctypes.data_as(P_l), len(idx),
                   _ptr(work), work.numel() * 8)

    # -- nearest-neighbour (Vecchia) path (include/fvgp_hip_nn.h) ---------------------------------------------------------------
    def _nn_check_idx_out(self, who, idx_out, nq):
        if idx_out.dim() != 2 or idx_out.stride(1) != 1 or idx_out.dtype != self.torch.int32 or idx_out.shape[0] < nq:
            raise ValueError(f"{who}: idx_out must be an int32 (nq, >= m) tensor with unit column stride, got {tuple(idx_out.shape)}")

    def nn_search(self, xq, xr, m, idx_out, scales=None, c0=-1):
        """fvgp_hip_nn_search: idx_out (nq, >= m) int32 device tensor <- per row of xq the m nearest candidates among the rows of xr,
        sorted by (distance, index), -1 past the candidate count; scales None or d positive numbers (host); c0 < 0: every row of xr is
        a candidate, c0 >= 0: rows j < min(nr, c0 + i) for query i.  Asynchronous."""
        self._nn_check_idx_out("nn_search", idx_out, xq.shape[0])
        sp = _scales_ptr("nn_search", scales, xq.shape[1])
        self._call("fvgp_hip_nn_search", _ptr(xq), xq.shape[0], _ptr(xr), xr.shape[0], xq.shape[1], sp, int(m), int(c0),
                   _ptr(idx_out), idx_out.stride(0))

    def nn_grid_build(self, xr, scales=None):
        """fvgp_hip_nn_grid_build: the cell grid over the rows of the device tensor xr (nr, d), d <= NN_GRID_MAX_DIM, under `scales`
        (None or d positive numbers, host) -> NNGrid.  Synchronises once (the bounding box is read back); the buffer is allocated
        here, the build's workspace is released with the call."""
        nr, d = xr.shape
        if not xr.is_contiguous() or xr.dtype != self.torch.float64:
            raise ValueError(f"nn_grid_build: xr must be a contiguous float64 (nr, d) tensor, got {tuple(xr.shape)} {xr.dtype}")
        if not 1 <= d <= NN_GRID_MAX_DIM:
            raise ValueError(f"nn_grid_build: the cell grid takes 1 .. {NN_GRID_MAX_DIM} dimensions, got {d}; nn_search has no such limit")
        sp = _scales_ptr("nn_grid_build", scales, d)
        buf = self.empty(max(1, nn_grid_bytes(nr, d)) // 8)
        work = self._work(None, "fvgp_hip_nn_grid_workspace_bytes", nr, d)
        info = np.zeros(NN_GRID_INFO)
        self._call("fvgp_hip_nn_grid_build", _ptr(xr), nr, d, sp, _ptr(buf), buf.numel() * 8, _ptr(work), work.numel() * 8,
                   info.ctypes.data_as(P_d))
        self.sync()                                # (the workspace goes back to the allocator with this frame)
        return NNGrid(buf, info, nr, d)

    def nn_grid_search(self, xq, xr, m, idx_out, grid, c0=-1):
        """fvgp_hip_nn_grid_search: idx_out as nn_search leaves it for (xq, xr, m, c0) under the scales `grid` (the NNGrid of
        nn_grid_build over this xr) was built with, element for element.  Asynchronous."""
        self._nn_check_idx_out("nn_grid_search", idx_out, xq.shape[0])
        if xq.shape[1] != xr.shape[1]:
            raise ValueError(f"nn_grid_search: xq has {xq.shape[1]} columns, xr {xr.shape[1]}")
        self._call("fvgp_hip_nn_grid_search", _ptr(xq), xq.shape[0], _ptr(xr), xr.shape[0], xr.shape[1], int(m), int(c0),
                   grid.info.ctypes.data_as(P_d), _ptr(grid.buffer), _ptr(idx_out), idx_out.stride(0))

    def nn_maxmin_order(self, x, first, q=None, scales=None, want_distances=True):
        """fvgp_hip_nn_maxmin_order: the exact maxmin ordering of the rows of the device tensor x (n, d) from the point `first`, its
        first q positions (default: all n), distances as in nn_search (scales None or d positive numbers, host).  Returns (perm (q,)
        int64 ndarray, dist (q,) float64 ndarray or None): dist[t] is the squared scaled distance of perm[t] to the nearest earlier pick,
        dist[0] = inf.  q launches in stream order, then one synchronisation for the results."""
        n, d = x.shape
        q = n if q is None else int(q)
        if not x.is_contiguous() or x.dtype != self.torch.float64:
            raise ValueError(f"nn_maxmin_order: x must be a contiguous float64 (n, d) tensor, got {tuple(x.shape)} {x.dtype}")
        sp = _scales_ptr("nn_maxmin_order", scales, d)
        perm = self.torch.empty((max(q, 1),), dtype=self.torch.int64, device=x.device)
        dist = self.empty(max(q, 1)) if want_distances else None
        work = self._work(None, "fvgp_hip_nn_maxmin_workspace_bytes", n)
        self._call("fvgp_hip_nn_maxmin_order", _ptr(x), n, d, sp, int(first), q, _ptr(perm), _ptr(dist), _ptr(work), work.numel() * 8)
        self.sync()
        return perm.cpu().numpy(), None if dist is None else dist.cpu().numpy()

    def _nn_operands(self, who, thetas, idx, nq, m, mu, var):
        t = np.ascontiguousarray(np.asarray(thetas, dtype=np.float64))
        t = t.reshape(1, -1) if t.ndim == 1 else t
        if t.ndim != 2:
            raise ValueError(f"{who}: thetas must be (B, ntheta)")
        B = t.shape[0]
        if idx.dim() != 2 or idx.stride(1) != 1 or idx.dtype != self.torch.int32 or idx.shape[0] < nq or idx.shape[1] < m:
            raise ValueError(f"{who}: idx must be an int32 (nq, >= m) tensor with unit column stride, got {tuple(idx.shape)}")
        for name, a in (("mu", mu), ("var", var)):
            if not a.is_contiguous() or a.numel() < B * nq:
                raise ValueError(f"{who}: {name} must be a contiguous (B, nq) tensor, got {tuple(a.shape)}")
        return t, B

    def nn_conditionals(self, kernel_id, xq, xr, thetas, idx, m, r, v, mu, var, s=None, work=None):
        """fvgp_hip_nn_conditionals: mu, var (B, nq) device tensors <- the conditional mean (without prior mean) and variance of every
        row of xq given its neighbours idx[i][:m] among the rows of xr, at the B rows of `thetas` (host, B x ntheta or one vector).
        r, v (nr): centred data and noise of the reference rows; s (nq) or None: added to every row's variance.  Returns info: 0, or
        1 + b nq + i of the first (b, i) whose variance is not positive (a failed pivot leaves NaN).  Synchronous."""
        nq = xq.shape[0]
        t, B = self._nn_operands("nn_conditionals", thetas, idx, nq, m, mu, var)
        work = self._work(work, "fvgp_hip_nn_workspace_bytes", NN_CONDITIONALS, nq, B)
        info = ctypes.c_int64(0)
        self._call("fvgp_hip_nn_conditionals", int(kernel_id), _ptr(xq), nq, _ptr(xr), xr.shape[0], xq.shape[1], t.ctypes.data_as(P_d),
                   t.shape[1], B, _ptr(idx), idx.stride(0), int(m), _ptr(r), _ptr(v), _ptr(s), _ptr(mu), _ptr(var),
                   _ptr(work), work.numel() * 8, ctypes.byref(info))
        return int(info.value)

    def _nn_likelihood(self, level, kernel_id, x, thetas, idx, m, r, v, mu, var, score, fisher_rows, work):
        """the three likelihood entries (level NN_VALUE, NN_GRAD, NN_FISHER): operand checks, workspace, host outputs and the call.
        Returns (out, grad, fisher, info), None where the level has none."""
        who = ("nn_loglik", "nn_loglik_grad", "nn_loglik_fisher")[level]
        n = x.shape[0]
        t, B = self._nn_operands(who, thetas, idx, n, m, mu, var)
        nth = t.shape[1]
        if level >= NN_GRAD and (not score.is_contiguous() or score.numel() < B * n * nth):
            raise ValueError(f"{who}: score must be a contiguous (B, n, ntheta) tensor, got {tuple(score.shape)}")
        if level == NN_FISHER and (not fisher_rows.is_contiguous() or fisher_rows.numel() < B * n * (nth * (nth + 1) // 2)):
            raise ValueError(f"{who}: fisher_rows must be a contiguous (B, n, ntheta (ntheta + 1) / 2) tensor, got "
                             f"{tuple(fisher_rows.shape)}")
        query = ("fvgp_hip_nn_workspace_bytes", NN_LOGLIK, n, B) if level == NN_VALUE else \
            ("fvgp_hip_nn_grad_workspace_bytes" if level == NN_GRAD else "fvgp_hip_nn_fisher_workspace_bytes", n, B, nth)
        work = self._work(work, *query)
        out = np.empty((B, 3), dtype=np.float64)
        grad = np.empty((B, nth), dtype=np.float64) if level >= NN_GRAD else None
        fisher = np.empty((B, nth, nth), dtype=np.float64) if level == NN_FISHER else None
        info = ctypes.c_int64(0)
        # the entries' argument lists differ by the arrays of their level alone: score, fisher_rows before work; grad, fisher behind out
        rows = [_ptr(a) for a in (score, fisher_rows)[:level]]
        sums = [a.ctypes.data_as(P_d) for a in (grad, fisher)[:level]]
        self._call("fvgp_hip_" + who, int(kernel_id), _ptr(x), n, x.shape[1], t.ctypes.data_as(P_d), nth, B, _ptr(idx), idx.stride(0), int(m),
                   _ptr(r), _ptr(v), _ptr(mu), _ptr(var), *rows, _ptr(work), work.numel() * 8, out.ctypes.data_as(P_d), *sums, ctypes.byref(info))
        return out, grad, fisher, int(info.value)

    def nn_loglik(self, kernel_id, x, thetas, idx, m, r, v, mu, var, work=None):
        """fvgp_hip_nn_loglik: the nearest-neighbour log-likelihood of the rows of x in their order (idx: nn_search of x on itself with
        c0 = 0) at the B rows of `thetas`.  Returns (out (B, 3) ndarray of {log p, sum (r - mu)^2 / var, sum log var}, info as
        nn_conditionals); mu, var (B, n) keep the per-row conditionals.  Synchronous."""
        out, _, _, info = self._nn_likelihood(NN_VALUE, kernel_id, x, thetas, idx, m, r, v, mu, var, None, None, work)
        return out, info

    def nn_loglik_grad(self, kernel_id, x, thetas, idx, m, r, v, mu, var, score, work=None):
        """fvgp_hip_nn_loglik_grad: nn_loglik and the exact gradient.  score (B, n, ntheta) device tensor <- every row's
        d log p(y_i | y_c(i)) / d theta.  Returns (out (B, 3) as nn_loglik, grad (B, ntheta) ndarray = d log p / d theta, info).
        Synchronous."""
        out, grad, _, info = self._nn_likelihood(NN_GRAD, kernel_id, x, thetas, idx, m, r, v, mu, var, score, None, work)
        return out, grad, info

    def nn_loglik_fisher(self, kernel_id, x, thetas, idx, m, r, v, mu, var, score, fisher_rows, work=None):
        """fvgp_hip_nn_loglik_fisher: nn_loglik_grad and the Fisher information of the product of conditionals.  fisher_rows
        (B, n, ntheta (ntheta + 1) / 2) device tensor <- every row's term, the packed lower triangle ((h, k <= h) at h (h + 1) / 2 + k).
        Returns (out (B, 3) and grad (B, ntheta) as nn_loglik_grad, fisher (B, ntheta, ntheta) ndarray = the rows' sum, symmetric, info).
        Synchronous."""
        return self._nn_likelihood(NN_FISHER, kernel_id, x, thetas, idx, m, r, v, mu, var, score, fisher_rows, work)

    # -- the nearest-neighbour factor as a preconditioner (include/fvgp_hip_nn.h) --------------------------------------
    def nn_transpose(self, idx, m=None):
        """the transposed lists of the device tensor idx (n, ld) int32, columns 0 .. m - 1 (default: all): built on the host
        (nn_transpose_lists: a stable sort, once per neighbour structure) and uploaded.  Returns (tr_start (n + 1), tr_pos (max(nnz, 1)))
        int64 device tensors and nnz; positions are i * ld + l with ld = idx.stride(0)."""
        n, ld = idx.shape[0], idx.stride(0)
        m = idx.shape[1] if m is None else int(m)
        host = np.full((n, ld), -1, dtype=np.int64)
        host[:, :m] = idx[:, :m].cpu().numpy()
        start, pos = nn_transpose_lists(host, n)
        dev = idx.device
        tr_pos = self.torch.zeros(max(len(pos), 1), dtype=self.torch.int64, device=dev)
        tr_pos[:len(pos)] = self.torch.as_tensor(pos, device=dev)
        return self.torch.as_tensor(start, device=dev), tr_pos, len(pos)

    def nn_factor(self, kernel_id, x, theta, idx, m, v, coef=None, dinv=None, transposed=None, work=None):
        """fvgp_hip_nn_factor: the rows of the sparse inverse Cholesky factor W of K(x, x) + diag(v) over the lists idx[i][:m] at ONE
        theta -- coef (n, ld = idx.stride(0)) and dinv (n), allocated here unless given (coef starts as zeros: its columns past m are
        never written).  transposed = (tr_start, tr_pos, nnz) of nn_transpose, built here when None.  Returns (NNFactor, info): info 0, or
        1 + the first row whose conditional variance is not positive.  Synchronous."""
        t, tp, nt = _theta(theta)
        n, d = x.shape
        if idx.dim() != 2 or idx.stride(1) != 1 or idx.dtype != self.torch.int32 or idx.shape[0] < n or idx.shape[1] < m:
            raise ValueError(f"nn_factor: idx must be an int32 (n, >= m) tensor with unit column stride, got {tuple(idx.shape)}")
        ld = idx.stride(0)
        if coef is None:
            coef = self.zeros(n, ld)
        if dinv is None:
            dinv = self.empty(n)
        if coef.stride(0) != ld or coef.stride(1) != 1:
            raise ValueError(f"nn_factor: coef must have idx's leading dimension {ld}, got stride {coef.stride()}")
        work = self._work(work, "fvgp_hip_nn_factor_workspace_bytes", n)
        info = ctypes.c_int64(0)
        self._call("fvgp_hip_nn_factor", int(kernel_id), _ptr(x), n, d, tp, nt, _ptr(idx), ld, int(m), _ptr(v), _ptr(coef), ld,
                   _ptr(dinv), _ptr(work), work.numel() * 8, ctypes.byref(info))
        tr_start, tr_pos, nnz = self.nn_transpose(idx, m) if transposed is None else transposed
        return NNFactor(idx, m, coef, dinv, tr_start, tr_pos, nnz), int(info.value)

    def nn_precond_apply(self, factor, R, Z, s=None, work=None):
        """fvgp_hip_nn_precond_apply: Z[:, :s] = W^T (W R[:, :s]) for the NNFactor `factor`, s <= PCG_MAX_RHS; R, Z (n, >= s) device
        tensors.  Asynchronous."""
        n = factor.dinv.shape[0]
        s = int(R.shape[1] if s is None else s)
        work = self._work(work, "fvgp_hip_nn_precond_apply_workspace_bytes", n)
        self._call("fvgp_hip_nn_precond_apply", n, *factor._args(), _ptr(R), R.stride(0), s, _ptr(Z), Z.stride(0),
                   _ptr(work), work.numel() * 8)

    def pcg_nn(self, kernel_id, x, theta, vdiag, B, X, factor, s=None, warm=False, tol=1e-10, max_iter=1000, check_every=8,
               max_restarts=3, work=None):
        """fvgp_hip_pcg_nn: Handle.pcg with z = W^T W r of the NNFactor `factor` as the preconditioner; x, vdiag, B, X in the factor's
        ordering.  Returns (iters, relres, status) as Handle.pcg does.  Synchronous."""
        t, tp, nt = _theta(theta)
        n, d = x.shape
        s = int(B.shape[1] if s is None else s)
        work = self._work(work, "fvgp_hip_pcg_nn_workspace_bytes", n)
        iters = np.zeros(max(s, 1), dtype=np.int32)
        status = np.zeros(max(s, 1), dtype=np.int32)
        relres = np.zeros(max(s, 1), dtype=np.float64)
        self._call("fvgp_hip_pcg_nn", int(kernel_id), _ptr(x), n, d, tp, nt, _ptr(vdiag), *factor._args(),
                   _ptr(B), B.stride(0), s, _ptr(X), X.stride(0), int(bool(warm)), float(tol), int(max_iter),
                   int(check_every), int(max_restarts), _ptr(work), work.numel() * 8,
                   iters.ctypes.data_as(P_i), relres.ctypes.data_as(P_d), status.ctypes.data_as(P_i))
        return iters[:s], relres[:s], status[:s]

    def posterior_prepare(self, L, n):
        """enqueue the inverted diagonal blocks the posterior's sweep substitutes with (fvgp_hip_posterior_prepare)"""
        self._call("fvgp_hip_posterior_prepare", _ptr(L), int(n), L.stride(0))

    def gemm(self, a_kmajor, b_nmajor, lower, M, N, K, alpha, A, B, beta, C):
        self._call("fvgp_hip_gemm", int(a_kmajor), int(b_nmajor), int(lower), M, N, K, float(alpha),
                   _ptr(A), A.stride(0), _ptr(B), B.stride(0), float(beta), _ptr(C), C.stride(0))

    def mfma_selftest(self, A, B, D):
        self._call("fvgp_hip_mfma_selftest", _ptr(A), _ptr(B), _ptr(D))

    def mfma_peak(self, out, blocks, iters):
        self._call("fvgp_hip_mfma_peak", _ptr(out), int(blocks), int(iters))

    def add_lower(self, A, n, B, alpha=1.0):
        """A[:n, :n] += alpha * B[:n, :n] on the lower triangle (K + V with a matrix-valued noise model)."""
        self._call("fvgp_hip_add_lower", _ptr(A), int(n), A.stride(0), _ptr(B), B.stride(0), float(alpha))

    def trace_dot(self, W, D, b, n):
        """sum_ij (W_ij - b_i b_j) D_ij over the full n x n arrays (W symmetric, both triangles valid); b a 1-d view or None."""
        out = ctypes.c_double(0.0)
        self._call("fvgp_hip_trace_dot", _ptr(W), W.stride(0), _ptr(D), D.stride(0), _ptr(b),
                   1 if b is None else b.stride(0), int(n), ctypes.byref(out))
        return out.value

    def add_matrix(self, A, B, alpha=1.0):
        """A += alpha * B on the rectangle of B's shape"""
        self._call("fvgp_hip_add_matrix", _ptr(A), A.stride(0), _ptr(B), B.stride(0), B.shape[0], B.shape[1], float(alpha))

    def dot(self, a, b, n):
        """sum of the elementwise products of the first n rows of two (rows, c) arrays"""
        out = ctypes.c_double(0.0)
        self._call("fvgp_hip_dot", _ptr(a), a.stride(0), _ptr(b), b.stride(0), int(n), a.shape[1], ctypes.byref(out))
        return out.value

    def coldot(self, A, B, rows, cols, out):
        self._call("fvgp_hip_coldot", _ptr(A), A.stride(0), _ptr(B), B.stride(0), int(rows), int(cols), _ptr(out))

    def colsumsq(self, V, out):
        """out[p] = sum_i V[i][p]^2 over the rows of V"""
        self._call("fvgp_hip_colsumsq", _ptr(V), V.shape[0], V.stride(0), V.shape[1], _ptr(out))

    def symmetrize(self, A, n):
        self._call("fvgp_hip_symmetrize", _ptr(A), int(n), A.stride(0))
