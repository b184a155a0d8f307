"""ctypes binding of libfsnap_hip.so (C ABI: include/fsnap_hip.h).

This is the ONLY way the Python host layer reaches the GPU.  There is no CPU fallback:
if the library is missing it is built with hipcc; if that is impossible, or no gfx950
device is present when a context is requested, a loud exception is raised.

ctypes releases the GIL for the duration of each foreign call (reference threading model:
single Python thread per rank).
"""
from __future__ import annotations

import ctypes
import os
from collections import namedtuple
from ctypes import POINTER, byref, c_char_p, c_double, c_int, c_int64, c_uint8, c_void_p

import numpy as np

from . import build as _build

# status codes (include/fsnap_hip.h)
OK = 0
E_ARG, E_HIP, E_STATE, E_NOMEM = -1, -2, -3, -4
NUM_NOT_SPD, NUM_SINGULAR, NUM_NONFINITE = 1, 2, 3
SOLVE_CHOL, SOLVE_LSTSQ, SOLVE_RIDGE, SOLVE_RIDGE_INV = 0, 1, 2, 3
SOLVE_LSTSQ_PROBE, SOLVE_RIDGE_PROBE, SOLVE_RIDGE_INV_PROBE = 4, 5, 6     # same, but an unresolved system comes back at once with rank = -1
PROBE_OF = {SOLVE_LSTSQ: SOLVE_LSTSQ_PROBE, SOLVE_RIDGE: SOLVE_RIDGE_PROBE, SOLVE_RIDGE_INV: SOLVE_RIDGE_INV_PROBE}
BASE_OF = {v: k for k, v in PROBE_OF.items()}
COMM_ID_BYTES = 128
REDUCE_SUM, REDUCE_MAX, REDUCE_MIN = 0, 1, 2
MERR_IID, MERR_ABC, MERR_FULL = 0, 1, 2
CAND_ERROR_SUMS, CAND_RHS = 0, 1            # fsnap_candidate_rows: what
UQ_QUAD, UQ_NORM = 0, 1                     # fsnap_row_variance: mode
SELECT_SUM, SELECT_MAX, SELECT_MEAN = 0, 1, 2   # fsnap_select_begin: objective
SELECT_OBJECTIVES = {"sum": SELECT_SUM, "max": SELECT_MAX, "mean": SELECT_MEAN}
INFL_SCORES, INFL_FULL = 0, 1                   # fsnap_influence_rows: mode
ROBUST_HUBER, ROBUST_BISQUARE, ROBUST_CAUCHY = 0, 1, 2   # fsnap_robust_reweight: loss
ROBUST_LOSSES = {"huber": ROBUST_HUBER, "bisquare": ROBUST_BISQUARE, "cauchy": ROBUST_CAUCHY}
OMP_OMP, OMP_OLS = 0, 1                         # fsnap_omp_gram / fsnap_omp_path: criterion
OMP_CRITERIA = {"omp": OMP_OMP, "ols": OMP_OLS}
BCS_REFERENCE, BCS_EXACT = 0, 1                 # fsnap_bcs_gram / fsnap_bcs_path: deletion
BCS_DELETIONS = {"reference": BCS_REFERENCE, "exact": BCS_EXACT}
BCS_RE, BCS_ADD, BCS_DEL, BCS_STOP = 0, 1, 2, 3  # the action of a pick
BCS_MAX_K, BCS_MAX_ACTIVE = 144, 64             # fsnap_bcs_path (the host route takes any)
SPEC_MAX_K = 144                                # fsnap_spectral_path (the host route takes any)
ROBUST_MAX_CLASSES = 32
MERR_METHODS = {"iid": MERR_IID, "abc": MERR_ABC, "full": MERR_FULL}

_P_D = POINTER(c_double)
_P_U8 = POINTER(c_uint8)

# name -> (restype, argtypes); the "exports every declared symbol" test walks this table
SIGNATURES = {
    "fsnap_version": (c_int, []),
    "fsnap_device_count": (c_int, [POINTER(c_int)]),
    "fsnap_ctx_create": (c_int, [c_int, POINTER(c_void_p)]),
    "fsnap_ctx_destroy": (c_int, [c_void_p]),
    "fsnap_ctx_set_stream": (c_int, [c_void_p, c_void_p]),
    "fsnap_ctx_use_own_stream": (c_int, [c_void_p]),
    "fsnap_set_option": (c_int, [c_void_p, c_char_p, c_int64]),
    "fsnap_last_error": (c_char_p, [c_void_p]),
    "fsnap_upload_rows": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p]),
    "fsnap_bind_rows": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p]),
    "fsnap_rows_alloc": (c_int, [c_void_p, c_int64, c_int64]),
    "fsnap_drop_rows": (c_int, [c_void_p]),
    "fsnap_assemble": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p,
                               c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int, c_int, c_int]),
    "fsnap_download_rows": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    "fsnap_set_weights": (c_int, [c_void_p, c_void_p, c_void_p]),
    "fsnap_set_weights_train": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    "fsnap_bind_weights": (c_int, [c_void_p, c_void_p, c_void_p]),
    "fsnap_normal_eq": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "fsnap_normal_eq_async": (c_int, [c_void_p, c_void_p]),
    "fsnap_normal_eq_resident": (c_int, [c_void_p, POINTER(c_void_p)]),
    "fsnap_download_packed": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
    "fsnap_mirror_packed": (c_int, [c_void_p, c_void_p, c_int64]),
    "fsnap_weight_rows": (c_int, [c_void_p, c_void_p, c_int64, c_void_p]),
    "fsnap_weight_rows_device": (c_int, [c_void_p, c_void_p, c_int64, c_void_p]),
    "fsnap_predict": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "fsnap_residual_rhs": (c_int, [c_void_p, c_void_p, c_void_p, POINTER(c_double)]),
    "fsnap_merr_eval": (c_int, [c_void_p, c_int, c_int64, c_void_p, c_void_p, c_double, POINTER(c_double), c_void_p,
                                c_void_p]),
    "fsnap_sse_batch": (c_int, [c_void_p, c_int64, c_void_p, c_int, c_void_p, POINTER(c_int64)]),
    "fsnap_solve": (c_int, [c_int, c_double, c_int64, c_void_p, c_void_p, c_void_p, POINTER(c_int), POINTER(c_double)]),
    "fsnap_cond_info": (c_int, [c_void_p]),
    "fsnap_lasso_gram": (c_int, [c_int64, c_void_p, c_void_p, c_double, c_double, c_int64, c_double, c_void_p,
                                 POINTER(c_int64), POINTER(c_double)]),
    "fsnap_omp_gram": (c_int, [c_int64, c_void_p, c_void_p, c_double, c_void_p, c_int, c_void_p, c_int64, c_int64, c_void_p,
                               c_void_p, c_void_p]),
    "fsnap_bcs_gram": (c_int, [c_int64, c_void_p, c_void_p, c_double, c_double, c_double, c_void_p, c_double, c_double, c_double,
                               c_int64, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                               c_void_p]),
    "fsnap_spectral_gram": (c_int, [c_int64, c_void_p, c_void_p, c_double, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p,
                                    c_void_p, c_void_p, c_void_p, c_void_p]),
    "fsnap_normal_eq_accumulate": (c_int, [c_void_p, c_void_p]),
    "fsnap_assemble_accumulate": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p,
                                          c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int, c_int, c_int,
                                          c_void_p]),
    "fsnap_error_stats": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "fsnap_solve_device": (c_int, [c_void_p, c_int, c_double, c_int64, c_void_p, c_void_p, POINTER(c_int), POINTER(c_double)]),
    "fsnap_fit_resident": (c_int, [c_void_p, c_int, c_double, c_void_p, POINTER(c_int), POINTER(c_double), POINTER(c_void_p)]),
    "fsnap_solve_device_rhs": (c_int, [c_void_p, c_int, c_double, c_int64, c_void_p, c_void_p, c_void_p, POINTER(c_int),
                                        POINTER(c_double)]),
    "fsnap_comm_id": (c_int, [c_void_p]),
    "fsnap_comm_id_p2p": (c_int, [c_void_p]),
    "fsnap_comm_transport": (c_int, [c_void_p, POINTER(c_int)]),
    "fsnap_comm_init": (c_int, [c_void_p, c_int, c_int, c_void_p]),
    "fsnap_comm_destroy": (c_int, [c_void_p]),
    "fsnap_comm_info": (c_int, [c_void_p, POINTER(c_int), POINTER(c_int)]),
    "fsnap_allreduce_device": (c_int, [c_void_p, c_void_p, c_int64]),
    "fsnap_allreduce_host": (c_int, [c_void_p, c_void_p, c_int64, c_int]),
    "fsnap_bcast_host": (c_int, [c_void_p, c_void_p, c_int64, c_int]),
    "fsnap_allgather_host": (c_int, [c_void_p, c_void_p, c_int64, c_void_p]),
    "fsnap_barrier": (c_int, [c_void_p]),
    "fsnap_fit_dist": (c_int, [c_void_p, c_int, c_double, c_int64, c_void_p, POINTER(c_int), POINTER(c_double), POINTER(c_void_p)]),
    "fsnap_dev_alloc": (c_int, [c_void_p, c_int64, POINTER(c_void_p)]),
    "fsnap_dev_free": (c_int, [c_void_p, c_void_p]),
    "fsnap_dev_sync": (c_int, [c_void_p]),
    "fsnap_dev_upload": (c_int, [c_void_p, c_void_p, c_void_p, c_int64]),
    "fsnap_dev_download": (c_int, [c_void_p, c_void_p, c_void_p, c_int64]),
    "fsnap_lstsq_rows": (c_int, [c_void_p, c_double, c_int64, c_void_p, POINTER(c_int), c_void_p]),
    "fsnap_set_dense_pinv": (c_int, [c_void_p, c_void_p, c_void_p]),
    "fsnap_trsm_pass": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, POINTER(c_int)]),
    "fsnap_qpack_device": (c_int, [c_void_p, c_void_p]),
    "fsnap_rowspace_factor": (c_int, [c_int64, c_void_p, c_int, c_double, c_void_p, c_void_p, c_void_p]),
    "fsnap_rowspace_solve": (c_int, [c_int64, c_void_p, c_void_p, c_double, c_void_p, POINTER(c_int), c_void_p]),
    "fsnap_timing": (c_int, [c_void_p, _P_D, c_int]),
    "fsnap_timing_history": (c_int, [c_void_p, c_void_p, c_void_p, c_int]),
    "fsnap_timing_count": (c_int, [c_void_p, c_void_p, c_void_p]),
    "fsnap_timing_history_comm": (c_int, [c_void_p, c_void_p, c_int]),
    "fsnap_rowspace_chain": (c_int, [c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_double, c_void_p, POINTER(c_int), c_void_p]),
    "fsnap_launch_info": (c_int, [c_void_p, POINTER(c_int64), c_int]),
    "fsnap_cat_chunks": (c_int, [c_int64, c_void_p, c_void_p, c_int, c_void_p, c_void_p, POINTER(c_int64)]),
    "fsnap_cat_info": (c_int, [c_void_p, POINTER(c_int64), c_int]),
    "fsnap_cat_prepare": (c_int, [c_void_p, c_void_p, c_int, POINTER(c_int64)]),
    "fsnap_cat_normal_eq": (c_int, [c_void_p, c_int64, POINTER(c_void_p)]),
    "fsnap_cat_normal_eq_dist": (c_int, [c_void_p, POINTER(c_int64), c_int64, c_int, POINTER(c_void_p)]),
    "fsnap_fit_candidates": (c_int, [c_void_p, c_int64, c_int, c_double, c_void_p, c_int, c_int, c_int64, c_void_p, c_void_p,
                                     c_void_p, POINTER(c_void_p)]),
    "fsnap_candidate_rows": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int, c_int, c_int64, c_int, c_void_p]),
    "fsnap_cv_candidates": (c_int, [c_void_p, c_int64, c_double, c_void_p, c_int, c_int, c_int, c_int64, c_void_p, c_void_p]),
    "fsnap_cv_candidate_rows": (c_int, [c_void_p, c_int64, c_void_p, c_int, c_int, c_int, c_int64, c_void_p]),
    "fsnap_cv_candidates_grad": (c_int, [c_void_p, c_int64, c_double, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int64,
                                         c_void_p, c_void_p, c_void_p, c_void_p]),
    "fsnap_cv_candidates_grad_rhs": (c_int, [c_void_p, c_int64, c_void_p]),
    "fsnap_cv_candidates_grad_times": (c_int, [c_void_p, c_void_p]),
    "fsnap_candidates_evidence": (c_int, [c_void_p, c_int64, c_double, c_void_p, c_int, c_int, c_int64, c_void_p, c_void_p, c_void_p,
                                          c_void_p]),
    "fsnap_candidates_evidence_times": (c_int, [c_void_p, c_void_p]),
    "fsnap_row_variance": (c_int, [c_void_p, c_int, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                                   c_void_p, c_void_p, c_void_p, c_void_p]),
    "fsnap_row_variance_device": (c_int, [c_void_p, c_int, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                          c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "fsnap_loco_rows": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p,
                                c_void_p]),
    "fsnap_loco_rows_uq": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p,
                                   c_void_p, c_void_p]),
    "fsnap_influence_rows": (c_int, [c_void_p, c_int, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p,
                                     c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "fsnap_ridge_path": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p,
                                 c_int64, c_void_p, c_void_p, c_void_p]),
    "fsnap_lasso_path": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_int64, c_int64, c_double, c_void_p,
                                 c_void_p, c_void_p]),
    "fsnap_ard_path": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_int64, c_int64, c_double, c_void_p,
                               c_void_p, c_void_p, c_void_p]),
    "fsnap_omp_path": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int, c_void_p, c_int64, c_int64, c_void_p,
                               c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "fsnap_bcs_path": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_int64, c_int64, c_int, c_void_p,
                               c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "fsnap_spectral_path": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p,
                                    c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "fsnap_spectral_path_times": (c_int, [c_void_p, c_void_p]),
    "fsnap_select_begin": (c_int, [c_void_p, c_int, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_int, c_int]),
    "fsnap_select_pick": (c_int, [c_void_p, c_int, POINTER(ctypes.c_int32), POINTER(c_double)]),
    "fsnap_select_retire": (c_int, [c_void_p, ctypes.c_int32]),
    "fsnap_select_downdate": (c_int, [c_void_p, c_int64, c_int64, c_void_p]),
    "fsnap_select_state": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "fsnap_select_end": (c_int, [c_void_p]),
    "fsnap_joint_begin": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "fsnap_joint_score": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_double, c_void_p, c_void_p,
                                  c_void_p]),
    "fsnap_joint_retire": (c_int, [c_void_p, c_int64]),
    "fsnap_joint_end": (c_int, [c_void_p]),
    "fsnap_robust_begin": (c_int, [c_void_p, c_void_p, c_int]),
    "fsnap_robust_residuals": (c_int, [c_void_p, c_void_p, c_int64]),
    "fsnap_robust_scale": (c_int, [c_void_p, c_void_p, c_void_p]),
    "fsnap_robust_reweight": (c_int, [c_void_p, c_int, c_double, c_void_p, c_void_p]),
    "fsnap_robust_step": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_double, c_void_p, c_void_p]),
    "fsnap_robust_download": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "fsnap_robust_end": (c_int, [c_void_p]),
}

_lib = None


class FsnapError(RuntimeError):
    """Runtime (HIP / state / argument) failure reported by libfsnap_hip."""


def _preload_torch_hip_runtime():
    """Keep ONE HIP runtime in the process.  PyTorch-ROCm wheels bundle their own libamdhip64
    (SONAME libamdhip64.so.7, requested by torch as plain ``libamdhip64.so``); if this library
    pulled in /opt/rocm's copy first, a later ``import torch`` would map a second runtime and
    its device enumeration fails ("No HIP GPUs are available").  Mapping torch's copy first
    makes both resolve to the same file, in either import order."""
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        return
    if spec is None or not spec.submodule_search_locations:
        return
    libdir = os.path.join(list(spec.submodule_search_locations)[0], "lib")
    cand = os.path.join(libdir, "libamdhip64.so")
    if os.path.exists(cand):
        try:
            ctypes.CDLL(cand, mode=ctypes.RTLD_GLOBAL)
        except OSError:
            return
        # the RCCL that belongs to that runtime (fsnap_comm.cpp loads it lazily, on the first fsnap_comm_* call)
        rccl = os.path.join(libdir, "librccl.so")
        if os.path.exists(rccl):
            os.environ.setdefault("FSNAP_RCCL_PATH", rccl)


def load_library(build_if_missing: bool = True):
    """Load (building first if needed) libfsnap_hip.so and attach prototypes."""
    global _lib
    if _lib is not None:
        return _lib
    # multi-process GPU work (RCCL) shares buffers through dmabuf IPC; the legacy IPC mode is not supported by the
    # host driver of the MI355X boxes (hipIpcGetMemHandle: invalid argument).  Must be set before the HSA runtime starts
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    _preload_torch_hip_runtime()
    path = _build.lib_path()
    if build_if_missing:
        path = _build.build_library()
    if not os.path.exists(path):
        raise FsnapError(f"libfsnap_hip.so not found at {path}; run `python -m fitsnap_amd.build`")
    lib = ctypes.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError here = symbol missing = broken build
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def _ptr(arr):
    return None if arr is None else arr.ctypes.data_as(c_void_p)


def _f64(x, name):
    a = np.ascontiguousarray(x, dtype=np.float64)
    if not a.flags["C_CONTIGUOUS"]:
        raise ValueError(f"{name} must be C-contiguous")
    return a


def raise_status(rc: int, msg: str):
    """Map a non-zero status to the exception class the reference would raise
    (np.linalg.LinAlgError / ValueError / MemoryError)."""
    if rc == OK:
        return
    if rc in (NUM_NOT_SPD, NUM_SINGULAR):
        raise np.linalg.LinAlgError(msg or ("matrix is not positive definite" if rc == NUM_NOT_SPD else "Singular matrix"))
    if rc == NUM_NONFINITE:
        raise ValueError(msg or "array must not contain infs or NaNs")
    if rc == E_NOMEM:
        raise MemoryError(msg or "device allocation failed")
    if rc == E_ARG:
        raise ValueError(msg or "bad argument")
    raise FsnapError(f"libfsnap_hip status {rc}: {msg}")


def device_count() -> int:
    lib = load_library()
    n = c_int(0)
    rc = lib.fsnap_device_count(byref(n))
    return n.value if rc == OK else 0


def solve(kind: int, param: float, G: np.ndarray, c: np.ndarray):
    """K x K back-solve on the host side of the library (no GPU needed).
    Returns (beta, rank, rcond_estimate)."""
    lib = load_library()
    G = _f64(G, "G")
    c = _f64(c, "c")
    K = c.shape[0]
    if G.shape != (K, K):
        raise ValueError("G must be K x K")
    beta = np.empty(K, dtype=np.float64)
    rank = c_int(0)
    rce = c_double(0.0)
    rc = lib.fsnap_solve(int(kind), float(param), K, _ptr(G), _ptr(c), _ptr(beta), byref(rank), byref(rce))
    raise_status(rc, "")
    return beta, rank.value, rce.value


def cond_info():
    """(smallest scaled pivot, lambda_min estimate from the factor, S^-1 applications, 0 host / 1 device factor) of the
    calling thread's last K x K solve (fsnap_cond_info)."""
    info = np.zeros(4)
    raise_status(load_library().fsnap_cond_info(_ptr(info)), "")
    return float(info[0]), float(info[1]), int(info[2]), int(info[3])


def lasso_gram(Q: np.ndarray, q: np.ndarray, y_norm2: float, l1_reg: float, max_iter: int = 2000, tol: float = 1.0e-4,
               start=None):
    """Cyclic coordinate descent for (1/2) w^T Q w - q^T w + l1_reg |w|_1 (fsnap_lasso_gram; host side, no GPU needed).
    Returns (w, sweeps, duality gap)."""
    lib = load_library()
    Q = _f64(Q, "Q")
    q = _f64(q, "q")
    K = q.shape[0]
    if Q.shape != (K, K):
        raise ValueError("Q must be K x K")
    w = np.zeros(K) if start is None else np.array(start, dtype=np.float64)
    if w.shape != (K,):
        raise ValueError("start must have K entries")
    nit = c_int64(0)
    gap = c_double(0.0)
    rc = lib.fsnap_lasso_gram(K, _ptr(Q), _ptr(q), float(y_norm2), float(l1_reg), int(max_iter), float(tol), _ptr(w),
                              byref(nit), byref(gap))
    raise_status(rc, "")
    return w, int(nit.value), float(gap.value)


def omp_criterion(criterion) -> int:
    """The criterion code of "omp" / "ols" (or of a code already); ValueError for anything else."""
    if isinstance(criterion, str) and criterion.lower() in OMP_CRITERIA:
        return OMP_CRITERIA[criterion.lower()]
    if not isinstance(criterion, (str, bool)) and criterion in (OMP_OMP, OMP_OLS):
        return int(criterion)
    raise ValueError(f"criterion must be one of {', '.join(OMP_CRITERIA)}, not {criterion!r}")


def omp_gram(Q: np.ndarray, q: np.ndarray, y2: float, steps: int, criterion="ols", forced=(), diag_ref=None):
    """Greedy forward selection on the statistics (fsnap_omp_gram; host side, no GPU needed): ``steps`` steps of orthogonal
    matching pursuit ("omp") or orthogonal least squares ("ols") after the ``forced`` columns.  ``diag_ref``: the diagonal the
    dead-column rule compares Q's with (None: Q's own).  Returns (order (steps, int32; -1 once the path has ended), path
    (steps x 3: e_s, score, pivot), coef (steps x K: the least-squares coefficients on the support of every step))."""
    lib = load_library()
    Q = _f64(Q, "Q")
    q = _f64(q, "q")
    K = q.shape[0]
    if Q.shape != (K, K):
        raise ValueError("Q must be K x K")
    ref = None if diag_ref is None else _f64(diag_ref, "diag_ref")
    if ref is not None and ref.shape != (K,):
        raise ValueError("diag_ref must have K entries")
    forced = np.ascontiguousarray(np.asarray(forced, dtype=np.int64).reshape(-1).astype(np.int32))
    S = int(steps)
    order = np.empty(max(S, 0), dtype=np.int32)
    path = np.empty((max(S, 0), 3))
    coef = np.empty((max(S, 0), K))
    rc = lib.fsnap_omp_gram(K, _ptr(Q), _ptr(q), float(y2), _ptr(ref), omp_criterion(criterion),
                            _ptr(forced) if forced.size else None, forced.size, S, _ptr(order), _ptr(path), _ptr(coef))
    raise_status(rc, "" if rc != E_ARG else f"fsnap_omp_gram: bad argument (K = {K}, steps = {S}, forced = {forced.tolist()})")
    return order, path, coef


def bcs_deletion(deletion) -> int:
    """The code of "reference" / "exact" (or of a code already); ValueError for anything else."""
    if isinstance(deletion, str) and deletion.lower() in BCS_DELETIONS:
        return BCS_DELETIONS[deletion.lower()]
    if not isinstance(deletion, (str, bool)) and deletion in (BCS_REFERENCE, BCS_EXACT):
        return int(deletion)
    raise ValueError(f"deletion must be one of {', '.join(BCS_DELETIONS)}, not {deletion!r}")


BcsFit = namedtuple("BcsFit", ["coef", "active", "alpha", "mu", "errbars", "Sig", "picks", "iterations", "status", "sigma2_in",
                               "sigma2", "rss", "margin"])


def bcs_gram(Q: np.ndarray, q: np.ndarray, y2: float, sum_y: float, n: float, sigma2=None, scale=0.01, eta=1e-18, itermax=10,
             max_active=0, deletion="reference", diag_ref=None):
    """BCS on the statistics (fsnap_bcs_gram; host side, no GPU needed): the reference's ``bcs()`` recurrence on Q = A^T A,
    q = A^T y, y2 = |y|^2, sum_y = sum y and n rows.  ``sigma2`` None: max(scale var(y), 1e-16); ``max_active`` 0: K;
    ``deletion`` "reference" (what the reference computes) or "exact" (Tipping & Faul's deletion); ``diag_ref``: the diagonal
    the dead-column rule compares Q's with (None: Q's own).  Returns a ``BcsFit``: coef (K), active (the columns in order),
    alpha, mu, errbars (by position), Sig (n_active x n_active, unclipped), picks (itermax x 2 int32: column, action 0
    re-estimate / 1 add / 2 delete / 3 chosen but stopped; -1 after the end), iterations, status (0 ended by a stop rule, 1
    failed -- NaN coefficients --, 2 itermax reached), sigma2_in, sigma2 (re-estimated), rss, margin."""
    lib = load_library()
    Q = _f64(Q, "Q")
    q = _f64(q, "q")
    K = q.shape[0]
    if Q.shape != (K, K):
        raise ValueError("Q must be K x K")
    ref = None if diag_ref is None else _f64(diag_ref, "diag_ref")
    if ref is not None and ref.shape != (K,):
        raise ValueError("diag_ref must have K entries")
    MA = int(max_active) if int(max_active) != 0 else K
    P = int(itermax)
    a = max(MA, 0)
    coef = np.empty(K)
    active = np.empty(a, dtype=np.int32)
    alpha, mu, err, Sig = np.empty(a), np.empty(a), np.empty(a), np.empty((a, a))
    picks = np.empty((max(P, 0), 2), dtype=np.int32)
    info = np.empty(6)
    rc = lib.fsnap_bcs_gram(K, _ptr(Q), _ptr(q), float(y2), float(sum_y), float(n), _ptr(ref),
                            0.0 if sigma2 is None else float(sigma2), float(scale), float(eta), P, MA, bcs_deletion(deletion),
                            _ptr(coef), _ptr(active), _ptr(alpha), _ptr(mu), _ptr(err), _ptr(Sig), _ptr(picks), _ptr(info))
    raise_status(rc, "" if rc != E_ARG else f"fsnap_bcs_gram: bad argument (K = {K}, sigma2 = {sigma2}, scale = {scale}, "
                                            f"eta = {eta}, itermax = {P}, max_active = {MA})")
    na = int(np.count_nonzero(active >= 0))
    return BcsFit(coef, active[:na].copy(), alpha[:na].copy(), mu[:na].copy(), err[:na].copy(), Sig[:na, :na].copy(), picks,
                  int(info[0]), int(info[1]), float(info[2]), float(info[3]), float(info[4]), float(info[5]))


SpectralFit = namedtuple("SpectralFit", ["eig", "z", "n_live", "sweeps", "off_ratio", "lambda_max", "lambda_min", "status", "rank",
                                         "dof", "sse", "coef"])


def spectral_gram(Q: np.ndarray, q: np.ndarray, y2: float, alphas, rconds, diag_ref=None):
    """Spectral path of one system on the statistics (fsnap_spectral_gram; host side, no GPU needed): one Jacobi
    eigendecomposition of the live block of Q = A^T A, then the fit of every setting (alpha, rcond) of the product grid, q =
    ia * len(rconds) + ir: g_i = z_i / (lambda_i + alpha) on the directions with lambda_i > max(rcond^2, 4 n_live eps)
    lambda_max.  ``diag_ref``: the diagonal the dead-column rule compares Q's with (None: Q's own).  Returns a
    ``SpectralFit``: eig and z (K, ascending, zero past n_live), n_live, sweeps, off_ratio, lambda_max, lambda_min, status (0
    converged, 2 sweep cap), rank, dof, sse (each Qa x Qr) and coef (Qa x Qr x K)."""
    lib = load_library()
    Q = _f64(Q, "Q")
    q = _f64(q, "q")
    K = q.shape[0]
    if Q.shape != (K, K):
        raise ValueError("Q must be K x K")
    ref = None if diag_ref is None else _f64(diag_ref, "diag_ref")
    if ref is not None and ref.shape != (K,):
        raise ValueError("diag_ref must have K entries")
    alphas = _f64(alphas, "alphas").reshape(-1)
    rconds = _f64(rconds, "rconds").reshape(-1)
    Qa, Qr = alphas.size, rconds.size
    eig, z, info = np.empty(K), np.empty(K), np.empty(6)
    sets = np.empty((Qa, Qr, 3))
    coef = np.empty((Qa, Qr, K))
    rc = lib.fsnap_spectral_gram(K, _ptr(Q), _ptr(q), float(y2), _ptr(ref), _ptr(alphas) if Qa else None, Qa,
                                 _ptr(rconds) if Qr else None, Qr, _ptr(eig), _ptr(z), _ptr(info), _ptr(sets), _ptr(coef))
    raise_status(rc, "" if rc != E_ARG else f"fsnap_spectral_gram: bad argument (K = {K}, alphas = {alphas.tolist()}, "
                                            f"rconds = {rconds.tolist()})")
    return SpectralFit(eig, z, int(info[0]), int(info[1]), float(info[2]), float(info[3]), float(info[4]), int(info[5]),
                       sets[:, :, 0].astype(np.int64), sets[:, :, 1].copy(), sets[:, :, 2].copy(), coef)


def rowspace_chain(factors, z, rcond, active=None):
    """K x K end of the row-space solve on factors kept apart (fsnap_rowspace_chain): returns (beta, rank, info)."""
    lib = load_library()
    R = _f64(np.ascontiguousarray(np.stack([np.asarray(f, dtype=np.float64) for f in factors])), "factors")
    nfac, K = R.shape[0], R.shape[1]
    z = _f64(z, "z")
    act = None if active is None else np.ascontiguousarray(np.asarray(active, dtype=np.uint8))
    beta = np.empty(K)
    rank = c_int(0)
    info = np.zeros(4)
    raise_status(lib.fsnap_rowspace_chain(K, nfac, _ptr(R), None if act is None else _ptr(act), _ptr(z), float(rcond), _ptr(beta),
                                          byref(rank), _ptr(info)), "")
    return beta, rank.value, {"chain": info[0], "norm_bound": info[1], "inverse_norm_bound": info[2], "cond_bound": info[3]}


DENSE_PINV_FN = ctypes.CFUNCTYPE(c_int, c_void_p, c_int64, c_int64, POINTER(c_double), c_double, POINTER(c_double),
                                 POINTER(c_double), POINTER(c_int))


def make_dense_pinv():
    """The hook ``fsnap_set_dense_pinv`` takes (include/fsnap_hip.h): x = pinv_rcond(T) y through LAPACK's divide-and-conquer
    SVD (scipy.linalg.svd, gesdd), the decomposition cached per ``token`` -- the K x K end of dgelsd for factors too large
    for the library's Jacobi sweeps.  Returns the ctypes callback object (keep it alive while it is installed)."""
    cache = {}

    def pinv_apply(user, token, n, T_p, rcond, y_p, x_p, rank_p):
        try:
            import scipy.linalg as sl

            n = int(n)
            held = cache.get("svd")
            if held is None or held[0] != (token, n):
                from ._hostblas import blas_threads

                T = np.ctypeslib.as_array(T_p, shape=(n, n))
                with blas_threads(n):               # (a BLAS pool sized by the CPUs it SEES is throttled behind a cgroup quota)
                    U, sv, Vt = sl.svd(T, full_matrices=False, lapack_driver="gesdd")
                keep = sv > rcond * sv[0] if (n and sv[0] > 0.0) else np.zeros(n, dtype=bool)   # gelsd's cut
                held = ((token, n), U[:, keep].copy(), sv[keep].copy(), Vt[keep].copy())
                cache["svd"] = held
            _, Uk, sk, Vk = held
            y = np.ctypeslib.as_array(y_p, shape=(n,))
            x = np.ctypeslib.as_array(x_p, shape=(n,))
            x[:] = Vk.T @ ((Uk.T @ y) / sk)
            rank_p[0] = int(sk.size)
            return 0
        except Exception:       # noqa: BLE001 - any failure: the library falls back on its own SVD
            return 1

    return DENSE_PINV_FN(pinv_apply)


TRANSPORTS = ("none", "rccl", "p2p")


def _cat_info(lib, handle):
    info = (c_int64 * 5)()
    rc = lib.fsnap_cat_info(handle, info, 5)
    if rc != OK:
        raise_status(rc, "fsnap_cat_info failed")
    return {"layout": info[0], "ncat": info[1], "K": info[2], "chunk_rows": info[3], "max_p": info[4]}


def cat_limits():
    """The candidate kernels' fixed sizes as the library has them: {"chunk_rows": rows per chunk, "max_p": candidates per
    launch of the row kernel}."""
    info = _cat_info(load_library(), None)
    return {"chunk_rows": info["chunk_rows"], "max_p": info["max_p"]}


def cat_chunks(cat, ncat: int, mask=None):
    """Host half of the candidate kernels' work layout (``fsnap_cat_chunks``): (sorted row ids, (n, 3) chunks of
    (category, first position, rows))."""
    lib = load_library()
    cat = np.ascontiguousarray(cat, dtype=np.int32)
    m = cat.shape[0]
    mk = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
    if mk is not None and mk.shape != (m,):
        raise ValueError("mask must have one entry per row")
    idx = np.empty(max(m, 1), dtype=np.int32)
    ch = np.empty((m + int(ncat), 3), dtype=np.int64)
    n = c_int64(0)
    rc = lib.fsnap_cat_chunks(m, _ptr(cat), _ptr(mk), int(ncat), _ptr(idx), _ptr(ch), byref(n))
    if rc != OK:
        raise_status(rc, (lib.fsnap_last_error(None) or b"").decode())
    nrows = int(ch[:n.value, 2].sum())
    return idx[:nrows].copy(), ch[:n.value].copy()


def comm_id(transport: str = None) -> bytes:
    """A fresh communicator id (rank 0 calls this and hands the 128 bytes to every rank).  ``transport``: "rccl", "p2p"
    (the one-shot peer-to-peer all-reduce over hipIpc windows, csrc/fsnap_p2p.cpp) or None = FSNAP_DIST_TRANSPORT, else
    RCCL.  The transport travels with the id: ``comm_init`` recognises it."""
    lib = load_library()
    buf = ctypes.create_string_buffer(COMM_ID_BYTES)
    if transport not in (None, "rccl", "p2p"):
        raise ValueError(f"unknown transport {transport!r}: 'rccl' or 'p2p'")
    if transport is None:
        transport = "p2p" if os.environ.get("FSNAP_DIST_TRANSPORT") == "p2p" else "rccl"
    if transport == "p2p":
        rc, name = lib.fsnap_comm_id_p2p(buf), "fsnap_comm_id_p2p"
    else:
        env = os.environ.pop("FSNAP_DIST_TRANSPORT", None)      # (fsnap_comm_id honours the variable by itself)
        try:
            rc, name = lib.fsnap_comm_id(buf), "fsnap_comm_id"
        finally:
            if env is not None:
                os.environ["FSNAP_DIST_TRANSPORT"] = env
    if rc != OK:
        raise FsnapError(f"{name}: " + (lib.fsnap_last_error(None) or b"").decode())
    return buf.raw


def rowspace_factor(G, Rhat=None, tol=1.0e-10):
    """Host step of a row-space pass (fsnap_rowspace_factor): returns (Rp or None when converged, Rhat, info) with
    info = (deviation, converged, shift).  ``Rhat=None`` starts a new factorisation."""
    lib = load_library()
    G = _f64(G, "G")
    K = G.shape[0]
    first = Rhat is None
    Rhat = np.zeros((K, K)) if first else _f64(Rhat, "Rhat")
    Rp = np.empty((K, K))
    info = np.zeros(3)
    raise_status(lib.fsnap_rowspace_factor(K, _ptr(G), int(first), float(tol), _ptr(Rhat), _ptr(Rp), _ptr(info)), "")
    return (None if info[1] else Rp), Rhat, tuple(info)


def rowspace_solve(Rhat, z, rcond=1.0e-13):
    """K x K end of the row-space solve (fsnap_rowspace_solve): returns (beta, rank, info)."""
    lib = load_library()
    Rhat = _f64(Rhat, "Rhat")
    z = _f64(z, "z")
    K = z.shape[0]
    beta = np.empty(K)
    rank = c_int(0)
    info = np.zeros(4)
    raise_status(lib.fsnap_rowspace_solve(K, _ptr(Rhat), _ptr(z), float(rcond), _ptr(beta), byref(rank), _ptr(info)), "")
    return beta, rank.value, tuple(info)


class HipContext:
    """One GPU's resident copy of (A, b, w, mask) and the kernels that run on it."""

    def __init__(self, device: int = 0):
        self._lib = load_library()
        self._h = c_void_p(None)
        rc = self._lib.fsnap_ctx_create(int(device), byref(self._h))
        if rc != OK:
            msg = (self._lib.fsnap_last_error(None) or b"").decode()
            raise FsnapError(f"cannot create a gfx950 context on device {device}: {msg} "
                             "(the HIP path is mandatory; there is no CPU fallback)")
        self.device = device
        self.m = 0
        self.K = 0
        self._keep = []  # keep numpy buffers alive across async copies
        self.resident_train_mask = None   # mask object last sent with set_weights_train (identity = still resident)
        # LAPACK's SVD for the large truncated K x K solves of the row-space path (the library's own is a Jacobi SVD)
        self._dense_pinv = make_dense_pinv()
        self._lib.fsnap_set_dense_pinv(self._h, ctypes.cast(self._dense_pinv, c_void_p), None)

    # -- plumbing --------------------------------------------------------------------
    def _check(self, rc):
        if rc != OK:
            raise_status(rc, (self._lib.fsnap_last_error(self._h) or b"").decode())

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.fsnap_ctx_destroy(self._h)
            self._h = c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_stream(self, stream_handle):
        self._check(self._lib.fsnap_ctx_set_stream(self._h, c_void_p(stream_handle or None)))

    def use_own_stream(self):
        self._check(self._lib.fsnap_ctx_use_own_stream(self._h))

    def set_option(self, key: str, value: int):
        self._check(self._lib.fsnap_set_option(self._h, key.encode(), int(value)))

    # -- rows / weights ----------------------------------------------------------------
    def upload_rows(self, A: np.ndarray, b: np.ndarray):
        A = np.asarray(A)
        if A.dtype != np.float64 or A.ndim != 2:
            A = np.ascontiguousarray(A, dtype=np.float64)
            if A.ndim != 2:
                raise ValueError("A must be 2-D")
        if A.strides[1] != 8 or A.strides[0] % 8 or A.strides[0] < A.shape[1] * 8:
            A = np.ascontiguousarray(A)
        b = _f64(b, "b")
        m, K = A.shape
        if b.shape != (m,):
            raise ValueError(f"b has shape {b.shape}, expected ({m},)")
        lda = A.strides[0] // 8
        self._check(self._lib.fsnap_upload_rows(self._h, _ptr(A), m, K, lda, _ptr(b)))
        if m != self.m:
            self.resident_train_mask = None
        self.m, self.K = m, K

    def bind_rows(self, dA_ptr: int, m: int, K: int, lda: int, db_ptr: int):
        self._check(self._lib.fsnap_bind_rows(self._h, c_void_p(dA_ptr), m, K, lda, c_void_p(db_ptr)))
        self.m, self.K = m, K

    def drop_rows(self):
        """No rows on this context any more (a rank of a multi-GPU job that owns none for the next fit)."""
        self._check(self._lib.fsnap_drop_rows(self._h))
        self.m = 0
        self.resident_train_mask = None

    def rows_alloc(self, m: int, K: int):
        self._check(self._lib.fsnap_rows_alloc(self._h, int(m), int(K)))
        self.m, self.K = int(m), int(K)

    def assemble(self, raw, row0, src_row, kind, frac, d, truth, weight, fractions, blank2J, ntypes, ncoeff, offcol):
        """Batch `_collect_lammps` transform into resident rows [row0, row0 + len(src_row))."""
        raw = np.ascontiguousarray(raw, dtype=np.float64)
        src_row = np.ascontiguousarray(src_row, dtype=np.int64)
        kind = np.ascontiguousarray(kind, dtype=np.int32)
        frac = np.ascontiguousarray(frac, dtype=np.int32)
        d = np.ascontiguousarray(d, dtype=np.float64)
        truth = np.ascontiguousarray(truth, dtype=np.float64)
        weight = np.ascontiguousarray(weight, dtype=np.float64)
        fractions = np.ascontiguousarray(fractions, dtype=np.float64).reshape(-1, ntypes)
        blank2J = np.ascontiguousarray(blank2J, dtype=np.float64)
        n = len(src_row)
        if not (len(kind) == len(frac) == len(d) == len(truth) == len(weight) == n):
            raise ValueError("plan arrays must have equal length")
        self._check(self._lib.fsnap_assemble(
            self._h, _ptr(raw), raw.shape[0], raw.shape[1], n, int(row0), _ptr(src_row), _ptr(kind), _ptr(frac), _ptr(d),
            _ptr(truth), _ptr(weight), _ptr(fractions) if fractions.size else None, fractions.shape[0], _ptr(blank2J),
            int(ntypes), int(ncoeff), int(offcol)))

    def assemble_accumulate(self, raw, src_row, kind, frac, d, truth, weight, fractions, blank2J, ntypes, ncoeff, offcol,
                            d_packed_ptr: int):
        """`process_single` + `c += aw.T @ aw; d += aw.T @ bw` (transpose_trick/example.py:230-237) for a batch, with the
        rows formed in registers: the packed statistics at ``d_packed_ptr`` (device) += those of the batch."""
        raw = np.ascontiguousarray(raw, dtype=np.float64)
        src_row = np.ascontiguousarray(src_row, dtype=np.int64)
        kind = np.ascontiguousarray(kind, dtype=np.int32)
        frac = np.ascontiguousarray(frac, dtype=np.int32)
        d = np.ascontiguousarray(d, dtype=np.float64)
        truth = np.ascontiguousarray(truth, dtype=np.float64)
        weight = np.ascontiguousarray(weight, dtype=np.float64)
        fractions = np.ascontiguousarray(fractions, dtype=np.float64).reshape(-1, ntypes)
        blank2J = np.ascontiguousarray(blank2J, dtype=np.float64)
        n = len(src_row)
        if not (len(kind) == len(frac) == len(d) == len(truth) == len(weight) == n):
            raise ValueError("plan arrays must have equal length")
        if raw.ndim != 2 or len(blank2J) != ntypes * (ncoeff + offcol):
            raise ValueError("raw must be 2-d and blank2J must have ntypes * (ncoeff + offcol) entries")
        self._check(self._lib.fsnap_assemble_accumulate(
            self._h, _ptr(raw), raw.shape[0], raw.shape[1], n, _ptr(src_row), _ptr(kind), _ptr(frac), _ptr(d),
            _ptr(truth), _ptr(weight), _ptr(fractions) if fractions.size else None, fractions.shape[0], _ptr(blank2J),
            int(ntypes), int(ncoeff), int(offcol), c_void_p(d_packed_ptr)))

    def download_rows(self, want_a=True, want_b=True, want_w=True, out_a=None, out_b=None, out_w=None):
        A = (out_a if out_a is not None else np.empty((self.m, self.K))) if want_a else None
        b = (out_b if out_b is not None else np.empty(self.m)) if want_b else None
        w = (out_w if out_w is not None else np.empty(self.m)) if want_w else None
        lda = (A.strides[0] // 8) if A is not None else self.K
        self._check(self._lib.fsnap_download_rows(self._h, _ptr(A), lda, _ptr(b), _ptr(w)))
        return A, b, w

    def set_weights(self, w: np.ndarray, mask=None):
        w = _f64(w, "w")
        if w.shape != (self.m,):
            raise ValueError(f"w has shape {w.shape}, expected ({self.m},)")
        mk = None
        if mask is not None:
            mk = np.ascontiguousarray(mask, dtype=np.uint8)
            if mk.shape != (self.m,):
                raise ValueError(f"mask has shape {mk.shape}, expected ({self.m},)")
        self._check(self._lib.fsnap_set_weights(self._h, _ptr(w), _ptr(mk)))
        if mk is not None:
            self.resident_train_mask = None          # the device mask buffer was overwritten

    def set_weights_train(self, w_train: np.ndarray, mask=None, rank=None):
        """One weight per TRAINING row (fsnap_set_weights_train); ``mask`` (uint8, 1 = train) and ``rank`` (int32
        exclusive prefix sum of the mask) go along the first time and whenever the training set changes, ``None``
        keeps the resident ones."""
        w_train = _f64(w_train, "w")
        mk = rk = None
        if mask is not None:
            mk = np.ascontiguousarray(mask, dtype=np.uint8)
            rk = np.ascontiguousarray(rank, dtype=np.int32)
            if mk.shape != (self.m,) or rk.shape != (self.m,):
                raise ValueError(f"mask / rank must have shape ({self.m},)")
        self._check(self._lib.fsnap_set_weights_train(self._h, _ptr(w_train), w_train.shape[0], _ptr(mk), _ptr(rk)))
        if mask is not None:
            self.resident_train_mask = mask          # the object whose content is on the device now

    def bind_weights(self, dw_ptr: int, dmask_ptr: int = 0):
        self._check(self._lib.fsnap_bind_weights(self._h, c_void_p(dw_ptr), c_void_p(dmask_ptr or None)))

    # -- hot path ----------------------------------------------------------------------
    def normal_eq(self):
        """Returns (G, c, scalars) on the host; scalars = [bw.bw, sum(bw), n_train]."""
        K = self.K
        G = np.empty((K, K))
        c = np.empty(K)
        s = np.empty(3)
        self._check(self._lib.fsnap_normal_eq(self._h, _ptr(G), _ptr(c), _ptr(s)))
        return G, c, s

    def normal_eq_async(self, d_packed_ptr: int):
        self._check(self._lib.fsnap_normal_eq_async(self._h, c_void_p(d_packed_ptr)))

    def normal_eq_resident(self) -> int:
        """Statistics into the context-owned device buffer; returns its device address."""
        ptr = c_void_p(None)
        self._check(self._lib.fsnap_normal_eq_resident(self._h, byref(ptr)))
        return ptr.value

    def mirror_packed(self, d_packed_ptr: int, K: int):
        """Statistics in HBM (e.g. just all-reduced) -> page-locked host mirror, asynchronously; the next
        solve_device on the same pointer then needs no D2H copy."""
        self._check(self._lib.fsnap_mirror_packed(self._h, c_void_p(d_packed_ptr), int(K)))

    def download_packed(self, d_packed_ptr: int, K: int):
        G = np.empty((K, K))
        c = np.empty(K)
        s = np.empty(3)
        self._check(self._lib.fsnap_download_packed(self._h, c_void_p(d_packed_ptr), K, _ptr(G), _ptr(c), _ptr(s)))
        return G, c, s

    def weight_rows(self):
        aw = np.empty((self.m, self.K))
        bw = np.empty(self.m)
        self._check(self._lib.fsnap_weight_rows(self._h, _ptr(aw), self.K, _ptr(bw)))
        return aw, bw

    def weight_rows_device(self, d_aw_ptr: int, ldaw: int, d_bw_ptr: int):
        self._check(self._lib.fsnap_weight_rows_device(self._h, c_void_p(d_aw_ptr), ldaw, c_void_p(d_bw_ptr)))

    def predict(self, beta, want_preds=True, want_sse=False):
        beta = _f64(beta, "beta")
        if beta.shape != (self.K,):
            raise ValueError(f"beta has shape {beta.shape}, expected ({self.K},)")
        preds = np.empty(self.m) if want_preds else None
        sse = c_double(0.0)
        self._check(self._lib.fsnap_predict(self._h, _ptr(beta), _ptr(preds), byref(sse) if want_sse else None))
        return preds, (sse.value if want_sse else None)

    def residual_rhs(self, beta, want_sse=False):
        """s = (wA)^T (wb - wA beta) on the resident rows (refinement right-hand side)."""
        beta = _f64(beta, "beta")
        if beta.shape != (self.K,):
            raise ValueError(f"beta has shape {beta.shape}, expected ({self.K},)")
        s = np.empty(self.K)
        sse = c_double(0.0)
        self._check(self._lib.fsnap_residual_rhs(self._h, _ptr(beta), _ptr(s), byref(sse) if want_sse else None))
        return s, (sse.value if want_sse else None)

    def merr_eval(self, method, c, q, d):
        """MERR log-posterior pass over the resident training rows (``fsnap_merr_eval``): returns (val, g, h) with
        val = sum of the per-row terms (without the density's constants), g = dval/de x, h = dval/dv x o x summed over
        the rows.  method: "iid" / "abc" / "full" or a MERR_* code; q = sigma^2, zero outside the embedded columns."""
        code = MERR_METHODS.get(method, method) if isinstance(method, str) else int(method)
        if isinstance(method, str) and method not in MERR_METHODS:
            raise ValueError(f"unknown MERR method {method!r} (iid, abc or full)")
        c = _f64(c, "c")
        q = _f64(q, "q")
        if c.shape != (self.K,) or q.shape != (self.K,):
            raise ValueError(f"c / q have shapes {c.shape} / {q.shape}, expected ({self.K},)")
        val = c_double(0.0)
        g = np.empty(self.K)
        h = np.empty(self.K)
        self._check(self._lib.fsnap_merr_eval(self._h, code, self.K, _ptr(c), _ptr(q), float(d), byref(val), _ptr(g), _ptr(h)))
        return val.value, g, h

    SSE_MAX_P = 16

    def sse_batch(self, U):
        """Weighted residual sums of P <= 16 coefficient vectors (rows of U, P x K) over the resident training rows
        (``fsnap_sse_batch``): returns (sse[P], n_train) with sse[p] = sum (w (a . u_p - b))^2.  sse[p] depends on
        u_p and the rows only, whatever else is in the batch."""
        U = np.ascontiguousarray(U, dtype=np.float64)
        if U.ndim == 1:
            U = U.reshape(1, -1)
        if U.ndim != 2 or not 1 <= U.shape[0] <= self.SSE_MAX_P:
            raise ValueError(f"U has shape {U.shape}, expected (P, K) with 1 <= P <= {self.SSE_MAX_P}")
        sse = np.empty(U.shape[0])
        n = c_int64(0)
        self._check(self._lib.fsnap_sse_batch(self._h, U.shape[1], _ptr(U), U.shape[0], _ptr(sse), byref(n)))
        return sse, int(n.value)

    def normal_eq_accumulate(self, d_packed_ptr: int):
        """d_packed (device) += statistics of the resident rows (streaming / transpose-trick accumulation)."""
        self._check(self._lib.fsnap_normal_eq_accumulate(self._h, c_void_p(d_packed_ptr)))

    def error_stats(self, beta, cat, ncat: int):
        """Per-category sums of ``Solver.error_analysis`` for the resident rows (see fsnap_error_stats):
        returns an (ncat, 10) array."""
        beta = _f64(beta, "beta").reshape(-1)
        if beta.shape[0] != self.K:
            raise ValueError("beta must have K entries")
        if cat is not None:
            cat = np.ascontiguousarray(cat, dtype=np.int32)
            if cat.shape != (self.m,):
                raise ValueError("cat must have one entry per row")
            self.cat_serial = getattr(self, "cat_serial", 0) + 1    # identifies the categories now on the device
        stats = np.empty((int(ncat), 10), dtype=np.float64)
        self._check(self._lib.fsnap_error_stats(self._h, _ptr(beta), _ptr(cat), int(ncat), _ptr(stats)))
        return stats

    def fit_resident(self, kind: int, param: float):
        """Statistics + K x K solve of the resident rows in one library call; returns
        (beta, rank, rcond_estimate, device address of the packed statistics)."""
        beta = np.empty(self.K, dtype=np.float64)
        rank = c_int(0)
        rce = c_double(0.0)
        ptr = c_void_p()
        rc = self._lib.fsnap_fit_resident(self._h, int(kind), float(param), _ptr(beta), byref(rank), byref(rce), byref(ptr))
        if rc != OK:
            raise_status(rc, (self._lib.fsnap_last_error(self._h) or b"").decode() if rc < 0 else "")
        return beta, rank.value, rce.value, ptr.value

    def solve_device(self, kind: int, param: float, K: int, d_packed_ptr: int, rhs=None):
        """K x K solve from the packed statistics in HBM; returns (beta, rank, rcond_estimate).
        ``rhs`` (host, K doubles) replaces the c part of the packed buffer as right-hand side."""
        beta = np.empty(K, dtype=np.float64)
        rank = c_int(0)
        rce = c_double(0.0)
        if rhs is None:
            rc = self._lib.fsnap_solve_device(self._h, int(kind), float(param), int(K), c_void_p(d_packed_ptr), _ptr(beta),
                                              byref(rank), byref(rce))
        else:
            r = _f64(rhs, "rhs")
            if r.shape != (K,):
                raise ValueError("rhs must have K entries")
            rc = self._lib.fsnap_solve_device_rhs(self._h, int(kind), float(param), int(K), c_void_p(d_packed_ptr), _ptr(r),
                                                  _ptr(beta), byref(rank), byref(rce))
        if rc != OK:
            raise_status(rc, (self._lib.fsnap_last_error(self._h) or b"").decode() if rc < 0 else "")
        return beta, rank.value, rce.value

    # -- batched candidate fits (fsnap_cat_prepare ... fsnap_candidate_rows) ------------------------------------------
    def cat_prepare(self, cat, ncat: int) -> int:
        """Category layout of the resident rows, mask and weights (the weights become the base weights w0); returns the
        layout's tag, which every later call of the group names."""
        cat = np.ascontiguousarray(cat, dtype=np.int32)
        if cat.shape != (self.m,):
            raise ValueError("cat must have one entry per row")
        tag = c_int64(0)
        self._check(self._lib.fsnap_cat_prepare(self._h, _ptr(cat), int(ncat), byref(tag)))
        return tag.value

    def cat_info(self):
        """{"layout", "ncat", "K", "chunk_rows", "max_p"}: the layout the context holds now (fsnap_cat_info)."""
        return _cat_info(self._lib, self._h)

    def cat_normal_eq(self, layout: int) -> int:
        """Per-category statistics of the training rows; returns the device address of the ncat packed blocks."""
        ptr = c_void_p(None)
        self._check(self._lib.fsnap_cat_normal_eq(self._h, int(layout), byref(ptr)))
        return ptr.value

    def cat_normal_eq_dist(self, layout: int, K: int, ncat: int):
        """Collective form: the per-category statistics summed over the ranks, on every rank.  layout = 0 on a rank without
        rows.  Returns (layout tag, device address)."""
        ptr = c_void_p(None)
        tag = c_int64(int(layout))
        self._check(self._lib.fsnap_cat_normal_eq_dist(self._h, byref(tag), int(K), int(ncat), byref(ptr)))
        return tag.value, ptr.value

    def fit_candidates(self, layout: int, kind: int, param: float, S, K: int):
        """Combination + K x K solve of every candidate: (beta (P, K), rank (P,), rcond (P,), device address of the P
        packed buffers)."""
        S = np.ascontiguousarray(S, dtype=np.float64)
        if S.ndim != 2:
            raise ValueError("S must be (P, ncat)")
        P, ncat = S.shape
        beta = np.empty((P, int(K)))
        rank = np.empty(P, dtype=np.int32)
        rce = np.empty(P)
        ptr = c_void_p(None)
        rc = self._lib.fsnap_fit_candidates(self._h, int(layout), int(kind), float(param), _ptr(S), int(P), int(ncat), int(K),
                                            _ptr(beta), _ptr(rank), _ptr(rce), byref(ptr))
        if rc != OK:
            raise_status(rc, (self._lib.fsnap_last_error(self._h) or b"").decode() if rc < 0 else "")
        return beta, rank, rce, ptr.value

    def candidate_rows(self, layout: int, beta, S, what: int, ncat: int):
        """One pass over the rows for P coefficient vectors: (P, ncat, 4) error sums or (P, K) right-hand sides."""
        beta = np.ascontiguousarray(beta, dtype=np.float64)
        if beta.ndim != 2 or beta.shape[1] != self.K:
            raise ValueError(f"beta must have shape (P, {self.K})")
        P = beta.shape[0]
        Sa = None if S is None else np.ascontiguousarray(S, dtype=np.float64)
        if Sa is not None and Sa.shape != (P, int(ncat)):
            raise ValueError(f"S must have shape ({P}, {int(ncat)})")
        out = np.empty((P, int(ncat), 4) if what == CAND_ERROR_SUMS else (P, self.K))
        self._check(self._lib.fsnap_candidate_rows(self._h, int(layout), _ptr(beta), _ptr(Sa), int(P), int(ncat), self.K,
                                                   int(what), _ptr(out)))
        return out

    def cv_candidates(self, layout: int, alpha: float, S, F: int, K: int):
        """The P x F leave-one-fold-out refits of the candidates S (P, C) from the per-(fold, category) statistics the
        context holds for ``layout`` (``fsnap_cv_candidates``, K <= 144): (coef (P, F, K), info (P, F, 4): status, smallest
        scaled pivot, live columns, weighted training rows).  A failed problem has status 1 and NaN coefficients."""
        S = np.ascontiguousarray(S, dtype=np.float64)
        if S.ndim != 2:
            raise ValueError("S must be (P, C)")
        P, C = S.shape
        F, K = int(F), int(K)
        coef = np.empty((P, max(F, 0), max(K, 0)))
        info = np.empty((P, max(F, 0), 4))
        self._check(self._lib.fsnap_cv_candidates(self._h, int(layout), float(alpha), _ptr(S) if S.size else None, int(P), F,
                                                  int(C), K, _ptr(coef) if coef.size else None, _ptr(info) if info.size else None))
        return coef, info

    def cv_candidate_rows(self, layout: int, coef, C: int):
        """Held-out sums of P x F refits (``fsnap_cv_candidate_rows``): every categorised row of composite category
        fold * C + c against coef[p, fold]; (P, F * C, 4) = sum|r|, sum r^2, sum|w0 r|, sum (w0 r)^2."""
        coef = np.ascontiguousarray(coef, dtype=np.float64)
        if coef.ndim != 3 or coef.shape[2] != self.K:
            raise ValueError(f"coef must have shape (P, F, {self.K})")
        P, F, _ = coef.shape
        out = np.empty((P, F * int(C), 4))
        self._check(self._lib.fsnap_cv_candidate_rows(self._h, int(layout), _ptr(coef) if coef.size else None, int(P), int(F),
                                                      int(C), self.K, _ptr(out) if out.size else None))
        return out

    def cv_candidates_grad(self, layout: int, alpha: float, S, omega, coef, want_lambda=False):
        """The adjoint gradient of a cross-validated cost over the scales (``fsnap_cv_candidates_grad``, K <= 144): S and
        omega (P, C), coef (P, F, K) the refits of ``cv_candidates`` for the same layout, alpha and S.  Returns (grad_S (P, C) =
        dJ/dS, grad_log_alpha (P,), lambda (P, F, K) or None, info (P, F, 2): status, smallest scaled pivot).  A candidate
        with a status-1 problem has a NaN row."""
        S = np.ascontiguousarray(S, dtype=np.float64)
        omega = np.ascontiguousarray(omega, dtype=np.float64)
        coef = np.ascontiguousarray(coef, dtype=np.float64)
        if S.ndim != 2 or omega.shape != S.shape:
            raise ValueError("S and omega must both be (P, C)")
        P, C = S.shape
        if coef.ndim != 3 or coef.shape[0] != P:
            raise ValueError("coef must be (P, F, K)")
        F, K = coef.shape[1], coef.shape[2]
        grad = np.empty((P, C))
        gla = np.empty(P)
        lam = np.empty((P, F, K)) if want_lambda else None
        info = np.empty((P, F, 2))
        self._check(self._lib.fsnap_cv_candidates_grad(
            self._h, int(layout), float(alpha), _ptr(S) if S.size else None, _ptr(omega) if omega.size else None,
            _ptr(coef) if coef.size else None, int(P), int(F), int(C), int(K), _ptr(grad) if grad.size else None,
            _ptr(gla) if gla.size else None, _ptr(lam) if lam is not None and lam.size else None, _ptr(info) if info.size else None))
        return grad, gla, lam, info

    def cv_candidates_grad_times(self):
        """(V0 + G1 RHS, G2, G1 bilinear) device milliseconds of the last ``cv_candidates_grad`` call."""
        ms = np.empty(3)
        self._check(self._lib.fsnap_cv_candidates_grad_times(self._h, _ptr(ms)))
        return ms

    def cv_candidates_grad_rhs(self, P: int, F: int, K: int):
        """g (P, F, K), the adjoint right-hand sides of the last ``cv_candidates_grad`` call (tests and diagnostics)."""
        g = np.empty((int(P), int(F), int(K)))
        self._check(self._lib.fsnap_cv_candidates_grad_rhs(self._h, g.size, _ptr(g)))
        return g

    def candidates_evidence(self, layout: int, alpha: float, S, active, K: int):
        """The per-candidate solves and per-category terms of the evidence (``fsnap_candidates_evidence``, K <= 144): S and
        active (P, ncat).  Returns (beta (P, K), info (P, 6): status, smallest scaled pivot, live columns, log|H|, tr(H^-1), 0,
        terms (P, ncat, 2): tr(H^-1 G_c) and bb_c - 2 beta . r_c + beta' G_c beta)."""
        S = np.ascontiguousarray(S, dtype=np.float64)
        active = np.ascontiguousarray(active, dtype=np.uint8)
        if S.ndim != 2 or active.shape != S.shape:
            raise ValueError("S and active must both be (P, ncat)")
        P, ncat = S.shape
        K = int(K)
        beta = np.empty((P, max(K, 0)))
        info = np.empty((P, 6))
        terms = np.empty((P, ncat, 2))
        self._check(self._lib.fsnap_candidates_evidence(
            self._h, int(layout), float(alpha), _ptr(S) if S.size else None, int(P), int(ncat), K,
            _ptr(active) if active.size else None, _ptr(beta) if beta.size else None, _ptr(info) if info.size else None,
            _ptr(terms) if terms.size else None))
        return beta, info, terms

    def candidates_evidence_times(self):
        """(E1, E2 + E3) device milliseconds of the last ``candidates_evidence`` call."""
        ms = np.empty(2)
        self._check(self._lib.fsnap_candidates_evidence_times(self._h, _ptr(ms)))
        return ms

    # -- row-space least squares --------------------------------------------------------
    def row_variance(self, M, mode=UQ_QUAD, beta=None, scale=None, cat=None, ncat=0, want_var=True, want_preds=False):
        """One pass over the resident rows (``fsnap_row_variance``): var_i = a_i^T M a_i (``UQ_QUAD``, M is K x K) or
        ||a_i M||^2 (``UQ_NORM``, M is K x J), preds_i = a_i . beta, and with ``cat`` (one int id per row, negative = skip)
        per-category sum / max / count of scale_i var_i.  Returns a dict with "var", "preds", "cat_sum", "cat_max",
        "cat_count" (None where not asked for)."""
        mode = int(mode)
        M = _f64(M, "M")
        if M.ndim == 1:
            M = M.reshape(-1, 1)
        if M.ndim != 2:
            raise ValueError("M must be 2-D")
        K, J = M.shape
        m = self.m
        if beta is not None:
            beta = _f64(beta, "beta").reshape(-1)
            if beta.shape != (K,):
                raise ValueError(f"beta has shape {beta.shape}, expected ({K},)")
        elif want_preds:
            raise ValueError("want_preds needs beta")
        if scale is not None:
            scale = _f64(scale, "scale").reshape(-1)
            if scale.shape != (m,):
                raise ValueError(f"scale has shape {scale.shape}, expected ({m},)")
        ncat = int(ncat)
        sums = maxs = counts = None
        if cat is not None:
            cat = np.ascontiguousarray(cat, dtype=np.int32)
            if cat.shape != (m,):
                raise ValueError(f"cat has shape {cat.shape}, expected ({m},)")
            sums = np.empty(max(ncat, 0))
            maxs = np.empty(max(ncat, 0))
            counts = np.empty(max(ncat, 0), dtype=np.int64)
        var = np.empty(m) if want_var else None
        preds = np.empty(m) if want_preds else None
        self._check(self._lib.fsnap_row_variance(self._h, mode, K, J, _ptr(M), _ptr(beta), _ptr(scale), _ptr(cat), ncat,
                                                 _ptr(var), _ptr(preds), _ptr(sums), _ptr(maxs), _ptr(counts)))
        return {"var": var, "preds": preds, "cat_sum": sums, "cat_max": maxs, "cat_count": counts}

    def row_variance_device(self, M, mode, d_var=0, d_preds=0, beta=None, d_scale=0, cat=None, ncat=0, d_cat_sum=0,
                            d_cat_max=0, d_cat_count=0):
        """``fsnap_row_variance_device``: the same pass with device outputs (integer addresses, 0 = not wanted), queued on
        the context's stream."""
        M = _f64(M, "M")
        if M.ndim == 1:
            M = M.reshape(-1, 1)
        K, J = M.shape
        if beta is not None:
            beta = _f64(beta, "beta").reshape(-1)
        if cat is not None:
            cat = np.ascontiguousarray(cat, dtype=np.int32)
            if cat.shape != (self.m,):
                raise ValueError(f"cat has shape {cat.shape}, expected ({self.m},)")
        v = lambda p: c_void_p(p or None)    # noqa: E731
        self._check(self._lib.fsnap_row_variance_device(self._h, int(mode), K, J, _ptr(M), _ptr(beta), v(d_scale), _ptr(cat),
                                                        int(ncat), v(d_var), v(d_preds), v(d_cat_sum), v(d_cat_max),
                                                        v(d_cat_count)))

    # -- greedy batch selection (fsnap_select_*) ------------------------------------------
    def select_begin(self, M, mode=UQ_QUAD, scale=None, cat=None, ncat=0, objective=SELECT_SUM):
        """Start a selection session on the resident rows (``fsnap_select_begin``): the variances and category sums of
        ``row_variance(M, mode, scale=, cat=, ncat=)`` stay on the device; ``objective`` is SELECT_SUM / _MAX / _MEAN."""
        M = _f64(M, "M")
        if M.ndim == 1:
            M = M.reshape(-1, 1)
        if M.ndim != 2:
            raise ValueError("M must be 2-D")
        K, J = M.shape
        m = self.m
        if scale is not None:
            scale = _f64(scale, "scale").reshape(-1)
            if scale.shape != (m,):
                raise ValueError(f"scale has shape {scale.shape}, expected ({m},)")
        if cat is None:
            raise ValueError("select_begin needs categories")
        cat = np.ascontiguousarray(cat, dtype=np.int32)
        if cat.shape != (m,):
            raise ValueError(f"cat has shape {cat.shape}, expected ({m},)")
        self._check(self._lib.fsnap_select_begin(self._h, int(mode), K, J, _ptr(M), _ptr(scale), _ptr(cat) if m else None,
                                                 int(ncat), int(objective)))
        self._select_shape = (m, int(ncat))

    def select_pick(self, retire=True):
        """(category, score) of the best live category (``fsnap_select_pick``; category -1 when none is left); with
        ``retire`` it leaves the session."""
        c, s = ctypes.c_int32(-1), c_double(0.0)
        self._check(self._lib.fsnap_select_pick(self._h, int(bool(retire)), byref(c), byref(s)))
        return c.value, s.value

    def select_retire(self, category):
        """Take a live category out of the session (``fsnap_select_retire``)."""
        self._check(self._lib.fsnap_select_retire(self._h, int(category)))

    def select_downdate(self, V):
        """var_i -= ||a_i V||^2 on the session's resident variances, then the live categories' scores again
        (``fsnap_select_downdate``); V is K x J."""
        V = _f64(V, "V")
        if V.ndim == 1:
            V = V.reshape(-1, 1)
        if V.ndim != 2:
            raise ValueError("V must be 2-D")
        self._check(self._lib.fsnap_select_downdate(self._h, V.shape[0], V.shape[1], _ptr(V)))

    def select_state(self, want_var=True):
        """The session's state (``fsnap_select_state``): dict of "var", "cat_sum", "cat_max", "cat_count", "alive"."""
        m, ncat = getattr(self, "_select_shape", (0, 0))
        var = np.empty(m) if want_var else None
        sums, maxs = np.empty(ncat), np.empty(ncat)
        counts, alive = np.empty(ncat, dtype=np.int64), np.empty(ncat, dtype=np.int32)
        self._check(self._lib.fsnap_select_state(self._h, _ptr(var), _ptr(sums), _ptr(maxs), _ptr(counts), _ptr(alive)))
        return {"var": var, "cat_sum": sums, "cat_max": maxs, "cat_count": counts, "alive": alive.astype(bool)}

    def select_end(self):
        """Drop the selection session (``fsnap_select_end``)."""
        self._check(self._lib.fsnap_select_end(self._h))

    # -- joint unit scores (fsnap_joint_*) --------------------------------------------------
    def joint_begin(self, sorted_rows, unit_offsets, omega=None):
        """Start a joint-score session on the resident rows (``fsnap_joint_begin``): the rows of unit u are
        ``sorted_rows[unit_offsets[u]:unit_offsets[u + 1]]``, ``omega`` (one per resident row, None = 1) their weights."""
        rows = np.ascontiguousarray(sorted_rows, dtype=np.int32).reshape(-1)
        off = np.ascontiguousarray(unit_offsets, dtype=np.int64).reshape(-1)
        if off.size < 1:
            raise ValueError("unit_offsets needs nunits + 1 entries")
        if off[-1] != rows.size:
            raise ValueError(f"unit_offsets ends at {off[-1]}, sorted_rows has {rows.size} entries")
        if omega is not None:
            omega = _f64(omega, "omega").reshape(-1)
            if omega.shape != (self.m,):
                raise ValueError(f"omega has shape {omega.shape}, expected ({self.m},)")
        self._check(self._lib.fsnap_joint_begin(self._h, _ptr(rows) if rows.size else None, _ptr(off), off.size - 1, _ptr(omega)))
        self._joint_units = off.size - 1

    def joint_score(self, M, tau, B=None, want_gain=True, want_reduction=None):
        """Scores of the session's live units under C = M M^T (M: K x J) and noise variance ``tau`` (``fsnap_joint_score``):
        dict of "gain", "reduction" (None where not asked for; the reduction needs the target block B = M^T R^T, J x r) and
        "info" (nunits x 4: dim S, n space, smallest pivot, rows).  Units that are not alive get NaN."""
        M = _f64(M, "M")
        if M.ndim == 1:
            M = M.reshape(-1, 1)
        if M.ndim != 2:
            raise ValueError("M must be 2-D")
        K, J = M.shape
        r = 0
        if B is not None:
            B = _f64(B, "B")
            if B.ndim != 2 or B.shape[0] != J:
                raise ValueError(f"B must have shape ({J}, r)")
            r = B.shape[1]
        if want_reduction is None:
            want_reduction = B is not None
        nu = getattr(self, "_joint_units", 0)
        gain = np.empty(nu) if want_gain else None
        red = np.empty(nu) if want_reduction else None
        info = np.full((nu, 4), np.nan)
        self._check(self._lib.fsnap_joint_score(self._h, K, J, _ptr(M), r, _ptr(B) if r else None, float(tau), _ptr(gain),
                                                _ptr(red), _ptr(info)))
        return {"gain": gain, "reduction": red, "info": info}

    def joint_retire(self, unit):
        """Take a live unit out of the session (``fsnap_joint_retire``)."""
        self._check(self._lib.fsnap_joint_retire(self._h, int(unit)))

    def joint_end(self):
        """Drop the joint-score session (``fsnap_joint_end``)."""
        self._check(self._lib.fsnap_joint_end(self._h))

    # -- robust IRLS step (fsnap_robust_*) ---------------------------------------------------
    def robust_begin(self, cat=None, ncat=1):
        """Start a robust session on the resident rows and their current weights (``fsnap_robust_begin``): ``cat`` is one
        class id in [0, ncat) per resident row (None = one class)."""
        if cat is not None:
            cat = np.ascontiguousarray(cat, dtype=np.int32).reshape(-1)
            if cat.shape != (self.m,):
                raise ValueError(f"cat has shape {cat.shape}, expected ({self.m},)")
        self._check(self._lib.fsnap_robust_begin(self._h, _ptr(cat) if cat is not None and cat.size else None, int(ncat)))
        self._robust_shape = (self.m, int(ncat))

    def robust_residuals(self, beta):
        """e_i = w_i (b_i - a_i . beta) with the session's base weights, left on the device (``fsnap_robust_residuals``)."""
        beta = _f64(beta, "beta").reshape(-1)
        self._check(self._lib.fsnap_robust_residuals(self._h, _ptr(beta), beta.size))

    def robust_scale(self):
        """(scale, count) per class: 1.4826 x the exact median of |e| and the participating rows, over all ranks of a
        communicator (``fsnap_robust_scale``; collective there)."""
        ncat = getattr(self, "_robust_shape", (0, 1))[1]
        s, n = np.zeros(ncat), np.zeros(ncat, dtype=np.int64)
        self._check(self._lib.fsnap_robust_scale(self._h, _ptr(s), _ptr(n)))
        return s, n

    def _robust_args(self, loss, c, scale):
        ncat = getattr(self, "_robust_shape", (0, 1))[1]
        if isinstance(loss, str):
            if loss not in ROBUST_LOSSES:
                raise ValueError(f"unknown loss {loss!r}: one of {sorted(ROBUST_LOSSES)}")
            loss = ROBUST_LOSSES[loss]
        if scale is not None:
            scale = _f64(scale, "scale").reshape(-1)
            if scale.shape != (ncat,):
                raise ValueError(f"scale has shape {scale.shape}, expected ({ncat},)")
        return int(loss), float(c), scale, np.zeros((ncat, 6))

    def robust_reweight(self, loss, c, scale=None):
        """r = sqrt(omega) and w r from the session's residuals; the context's fits read w r from here on
        (``fsnap_robust_reweight``).  Returns this rank's per-class table (ncat x 6): n, rows with omega < 1, rows with
        omega = 0, sum omega, sum e^2, sum rho.  ``scale`` None = the scales of the last ``robust_scale``."""
        loss, c, scale, sums = self._robust_args(loss, c, scale)
        self._check(self._lib.fsnap_robust_reweight(self._h, loss, c, _ptr(scale), _ptr(sums)))
        return sums

    def robust_step(self, beta, loss, c, scale=None):
        """``robust_residuals`` + ``robust_reweight`` in one launch (``fsnap_robust_step``): the same bits, A read once."""
        beta = _f64(beta, "beta").reshape(-1)
        loss, c, scale, sums = self._robust_args(loss, c, scale)
        self._check(self._lib.fsnap_robust_step(self._h, _ptr(beta), beta.size, loss, c, _ptr(scale), _ptr(sums)))
        return sums

    def robust_download(self, e=True, r=False, wr=False):
        """Dict of the session's per-row vectors asked for: "e", "r", "wr" (``fsnap_robust_download``)."""
        m = getattr(self, "_robust_shape", (0, 1))[0]
        out = {k: np.zeros(m) for k, want in (("e", e), ("r", r), ("wr", wr)) if want}
        self._check(self._lib.fsnap_robust_download(self._h, _ptr(out.get("e")), _ptr(out.get("r")), _ptr(out.get("wr"))))
        return out

    def robust_end(self):
        """End the robust session: the context's weights and mask are those of ``robust_begin`` again
        (``fsnap_robust_end``)."""
        self._check(self._lib.fsnap_robust_end(self._h))

    def _loco_args(self, M, beta, sorted_rows, cfg_offsets):
        """(M, beta, rows, offsets, K, J, ncfg) of ``loco_rows`` / ``loco_rows_uq``, checked."""
        M = _f64(M, "M")
        if M.ndim == 1:
            M = M.reshape(-1, 1)
        if M.ndim != 2:
            raise ValueError("M must be 2-D")
        K, J = M.shape
        beta = _f64(beta, "beta").reshape(-1)
        if beta.shape != (K,):
            raise ValueError(f"beta has shape {beta.shape}, expected ({K},)")
        rows = np.ascontiguousarray(sorted_rows, dtype=np.int32).reshape(-1)
        off = np.ascontiguousarray(cfg_offsets, dtype=np.int64).reshape(-1)
        if off.size < 1:
            raise ValueError("cfg_offsets needs ncfg + 1 entries")
        ncfg = off.size - 1
        if off[-1] != rows.size:
            raise ValueError(f"cfg_offsets ends at {off[-1]}, sorted_rows has {rows.size} entries")
        return M, beta, rows, off, K, J, ncfg

    def loco_rows(self, M, beta, sorted_rows, cfg_offsets):
        """Leave-one-configuration-out predictions of the resident training rows (``fsnap_loco_rows``): M (K x J) with
        C = M M^T, the fit ``beta`` (K), the rows of configuration c at ``sorted_rows[cfg_offsets[c]:cfg_offsets[c + 1]]``.
        Returns (pred (m, NaN where a row is not listed or its configuration is not identifiable), info (ncfg x 4:
        d_c, smallest pivot, identifiable, n space))."""
        M, beta, rows, off, K, J, ncfg = self._loco_args(M, beta, sorted_rows, cfg_offsets)
        pred = np.empty(self.m)
        info = np.empty((ncfg, 4))
        self._check(self._lib.fsnap_loco_rows(self._h, K, J, _ptr(M), _ptr(beta), _ptr(rows) if rows.size else None,
                                              _ptr(off), ncfg, _ptr(pred), _ptr(info)))
        return pred, info

    def loco_rows_uq(self, M, beta, sorted_rows, cfg_offsets):
        """``loco_rows`` with the leave-out predictive variances (``fsnap_loco_rows_uq``).  Returns (pred, as ``loco_rows``
        bit for bit; leverage (m: q_i = a_i (G - X_c^T X_c + alpha I)^-1 a_i^T, NaN as pred); info (ncfg x 6: d_c, smallest
        pivot, identifiable, n space, log det H_c, e_c^T H_c^-1 e_c))."""
        M, beta, rows, off, K, J, ncfg = self._loco_args(M, beta, sorted_rows, cfg_offsets)
        pred = np.empty(self.m)
        lev = np.empty(self.m)
        info = np.empty((ncfg, 6))
        self._check(self._lib.fsnap_loco_rows_uq(self._h, K, J, _ptr(M), _ptr(beta), _ptr(rows) if rows.size else None,
                                                 _ptr(off), ncfg, _ptr(pred), _ptr(lev), _ptr(info)))
        return pred, lev, info

    def influence_rows(self, M, beta, sorted_rows, cfg_offsets, mode=INFL_FULL, want_pred=True, want_vectors=True,
                       want_sums=True):
        """Per-configuration influence vectors and the outer-product sums of the cluster-robust covariances
        (``fsnap_influence_rows``); arguments as ``loco_rows``.  ``mode``: ``INFL_FULL`` (s_c, v_c, W_s, W_v and the
        predictions) or ``INFL_SCORES`` (s_c and W_s alone: no factorisation).  Returns a dict: "info" (ncfg x 4, as
        ``loco_rows``; SCORES: d_c, inf, 1, n space), "unit" (ncfg x 3: |v_c|^2, |s_c|^2, s_c . v_c; first and third NaN when
        c is not identifiable or in SCORES mode), "S" (ncfg x J; None without ``want_vectors``), "Ws" (J x J; None without
        ``want_sums``) and, in FULL mode, "pred" (m, ``loco_rows``' bits; None without ``want_pred``), "V" (ncfg x J, zeros
        where c is not identifiable) and "Wv"."""
        M, beta, rows, off, K, J, ncfg = self._loco_args(M, beta, sorted_rows, cfg_offsets)
        if mode not in (INFL_SCORES, INFL_FULL):
            raise ValueError(f"mode {mode!r} (INFL_SCORES, INFL_FULL)")
        full = mode == INFL_FULL
        # without units or rows the entry point writes the sums only: the rest keeps what an empty layout means
        out = {"pred": np.full(self.m, np.nan) if full and want_pred else None,
               "info": np.tile(np.array([0.0, np.inf, 1.0, 1.0]), (ncfg, 1)),
               "unit": np.zeros((ncfg, 3)), "S": np.zeros((ncfg, J)) if want_vectors else None,
               "V": np.zeros((ncfg, J)) if full and want_vectors else None, "Ws": np.empty((J, J)) if want_sums else None,
               "Wv": np.empty((J, J)) if full and want_sums else None}
        self._check(self._lib.fsnap_influence_rows(self._h, mode, K, J, _ptr(M), _ptr(beta), _ptr(rows) if rows.size else None,
                                                   _ptr(off), ncfg, *(_ptr(out[k]) if out[k] is not None else None
                                                                      for k in ("pred", "info", "unit", "S", "V", "Ws", "Wv"))))
        return out

    def ridge_path(self, G, c, alphas, sorted_rows, unit_offsets, row_class, nclass, want_preds=False):
        """Leave-one-unit-out refits of the resident training rows over a grid of alphas (``fsnap_ridge_path``, K <= 144): the
        statistics G (K x K), c (K), the grid ``alphas`` (Q), the rows of unit u at
        ``sorted_rows[unit_offsets[u]:unit_offsets[u + 1]]``, ``row_class`` (m, uint8, < nclass <= 8).  Returns (sums
        (Q x nunits x nclass x 4: n, sum |r|, sum r^2, sum (w r)^2), info (Q x nunits x 2: smallest pivot, identifiable),
        preds (Q x m, NaN where a row is not listed or its unit is not identifiable; None without ``want_preds``))."""
        G = _f64(G, "G")
        if G.ndim != 2 or G.shape[0] != G.shape[1]:
            raise ValueError("G must be square")
        K = G.shape[0]
        c = _f64(c, "c").reshape(-1)
        if c.shape != (K,):
            raise ValueError(f"c has shape {c.shape}, expected ({K},)")
        alphas = _f64(alphas, "alphas").reshape(-1)
        rows = np.ascontiguousarray(sorted_rows, dtype=np.int32).reshape(-1)
        off = np.ascontiguousarray(unit_offsets, dtype=np.int64).reshape(-1)
        if off.size < 1:
            raise ValueError("unit_offsets needs nunits + 1 entries")
        nunits = off.size - 1
        if off[-1] != rows.size:
            raise ValueError(f"unit_offsets ends at {off[-1]}, sorted_rows has {rows.size} entries")
        cls = np.ascontiguousarray(row_class, dtype=np.uint8).reshape(-1)
        if cls.size != self.m:
            raise ValueError(f"row_class has {cls.size} entries for {self.m} rows")
        Q, nclass = alphas.size, int(nclass)
        sums = np.empty((Q, nunits, max(nclass, 0), 4))
        info = np.empty((Q, nunits, 2))
        preds = np.empty((Q, self.m)) if want_preds else None
        self._check(self._lib.fsnap_ridge_path(self._h, K, _ptr(G), _ptr(c), _ptr(alphas), Q, _ptr(rows) if rows.size else None,
                                               _ptr(off), nunits, _ptr(cls) if cls.size else None, nclass, _ptr(sums),
                                               _ptr(info), _ptr(preds) if want_preds else None))
        return sums, info, preds

    def lasso_path(self, d_stats_ptr: int, K: int, F: int, nsub: int, alphas, max_iter: int, tol: float):
        """Grouped K-fold LASSO alpha path on per-fold statistics in device memory (``fsnap_lasso_path``, K <= 144):
        ``d_stats_ptr`` is the device address of F * nsub packed blocks (``cat_normal_eq``), fold f the sum of ``nsub``
        consecutive ones.  Returns (coef ((F + 1) x Q x K; index F: no fold left out), info ((F + 1) x Q x 4: sweeps, last
        duality gap, l1_reg, n), heldout (F x Q x 3: n_f, weighted squared error of fold f under its own refit, bb_f))."""
        alphas = _f64(alphas, "alphas").reshape(-1)
        K, F, Q = int(K), int(F), alphas.size
        coef = np.empty((max(F, 0) + 1, Q, max(K, 0)))
        info = np.empty((max(F, 0) + 1, Q, 4))
        held = np.empty((max(F, 0), Q, 3))
        self._check(self._lib.fsnap_lasso_path(self._h, K, F, int(nsub), c_void_p(d_stats_ptr), _ptr(alphas) if Q else None, Q,
                                               int(max_iter), float(tol), _ptr(coef), _ptr(info), _ptr(held)))
        return coef, info, held

    def omp_path(self, d_stats_ptr: int, K: int, F: int, nsub: int, criterion, forced, steps: int, levels):
        """Grouped K-fold greedy forward-selection path on per-fold statistics in device memory (``fsnap_omp_path``, K <= 144,
        steps <= min(K, 128)): ``d_stats_ptr`` as for ``lasso_path``; ``criterion`` "omp" / "ols"; ``forced``: columns taken
        first, in order; ``levels``: the ascending step counts at which coefficients are returned.  Returns (order ((F + 1) x
        steps, int32; index F: no fold left out; -1 once a path has ended), path ((F + 1) x steps x 3: e_s, score, pivot),
        heldout (F x steps x 3: n_f, weighted squared error of fold f under its own refit after s steps, bb_f), coef ((F + 1)
        x Q x K at the levels))."""
        forced = np.ascontiguousarray(np.asarray(forced, dtype=np.int64).reshape(-1).astype(np.int32))
        levels = np.ascontiguousarray(np.asarray(levels, dtype=np.int64).reshape(-1).astype(np.int32))
        K, F, S, Q = int(K), int(F), int(steps), levels.size
        order = np.empty((max(F, 0) + 1, max(S, 0)), dtype=np.int32)
        path = np.empty((max(F, 0) + 1, max(S, 0), 3))
        held = np.empty((max(F, 0), max(S, 0), 3))
        coef = np.empty((max(F, 0) + 1, Q, max(K, 0)))
        self._check(self._lib.fsnap_omp_path(self._h, K, F, int(nsub), c_void_p(d_stats_ptr), omp_criterion(criterion),
                                             _ptr(forced) if forced.size else None, forced.size, S, _ptr(levels) if Q else None, Q,
                                             _ptr(order), _ptr(path), _ptr(held), _ptr(coef)))
        return order, path, held, coef

    def bcs_path(self, d_stats_ptr: int, K: int, F: int, nsub: int, hyper, max_active: int, deletion="reference"):
        """Grouped K-fold BCS sparsity path on per-fold statistics in device memory (``fsnap_bcs_path``, K <= 144, max_active
        <= min(K, 64)): ``d_stats_ptr`` as for ``lasso_path``; ``hyper`` (Q x 4: sigma2 or 0, scale, eta, itermax of every
        setting; sigma2 = 0: scale x the variance of the problem's own rows).  With P = the largest itermax, returns (coef
        ((F + 1) x Q x K; index F: no fold left out), active ((F + 1) x Q x max_active int32, -1 past the active set), alpha
        and errbars (the same shape, by position), picks ((F + 1) x Q x P x 2 int32), info ((F + 1) x Q x 6: iterations,
        status, sigma2 used, sigma2 re-estimated, rss, margin), heldout (F x Q x 3: n_f, weighted squared error of fold f
        under its own refit, bb_f), Sig (Q x max_active x max_active of the fits on all rows))."""
        hyper = _f64(hyper, "hyper")
        K, F, MA = int(K), int(F), int(max_active)
        if hyper.ndim != 2 or hyper.shape[1] != 4:
            raise ValueError(f"hyper must have shape (Q, 4), not {hyper.shape}")
        Q = hyper.shape[0]
        its = hyper[:, 3] if Q else np.zeros(0)
        P = int(its.max()) if Q and np.all(np.isfinite(its)) and its.max() >= 1 and its.max() <= 65536 else 1
        n1, a = max(F, 0) + 1, max(MA, 0)
        coef = np.empty((n1, Q, max(K, 0)))
        active = np.empty((n1, Q, a), dtype=np.int32)
        alpha, err = np.empty((n1, Q, a)), np.empty((n1, Q, a))
        picks = np.empty((n1, Q, P, 2), dtype=np.int32)
        info = np.empty((n1, Q, 6))
        held = np.empty((max(F, 0), Q, 3))
        Sig = np.empty((Q, a, a))
        self._check(self._lib.fsnap_bcs_path(self._h, K, F, int(nsub), c_void_p(d_stats_ptr), _ptr(hyper) if Q else None, Q, MA,
                                             bcs_deletion(deletion), _ptr(coef), _ptr(active), _ptr(alpha), _ptr(err),
                                             _ptr(picks), _ptr(info), _ptr(held), _ptr(Sig)))
        return coef, active, alpha, err, picks, info, held, Sig

    def spectral_path(self, d_stats_ptr: int, K: int, F: int, nsub: int, alphas, rconds, want_coef: bool = True):
        """Grouped K-fold spectral path on per-fold statistics in device memory (``fsnap_spectral_path``, K <= 144):
        ``d_stats_ptr`` as for ``lasso_path``; the settings are the product grid of ``alphas`` and ``rconds``, q = ia * Qr + ir.
        Returns (eig and z ((F + 1) x K, ascending, zero past n_live; index F: no fold left out), info ((F + 1) x 6: n_live,
        sweeps, final off / diag ratio, lambda_max, smallest lambda, status 0 converged / 2 sweep cap), sets ((F + 1) x Q x 3:
        rank, dof, sse), fits (Q x K, on all rows), coef (F x Q x K of the refits, or None without ``want_coef``), heldout (F
        x Q x nsub x 3: n, weighted squared error of class s of fold f under the fold's own refit, bb))."""
        alphas = _f64(alphas, "alphas").reshape(-1)
        rconds = _f64(rconds, "rconds").reshape(-1)
        K, F, nsub, Qa, Qr = int(K), int(F), int(nsub), alphas.size, rconds.size
        Q, n1, k = Qa * Qr, max(F, 0) + 1, max(K, 0)
        eig, z, info = np.empty((n1, k)), np.empty((n1, k)), np.empty((n1, 6))
        sets = np.empty((n1, Q, 3))
        fits = np.empty((Q, k))
        coef = np.empty((max(F, 0), Q, k)) if want_coef else None
        held = np.empty((max(F, 0), Q, max(nsub, 0), 3))
        self._check(self._lib.fsnap_spectral_path(self._h, K, F, nsub, c_void_p(d_stats_ptr), _ptr(alphas) if Qa else None, Qa,
                                                  _ptr(rconds) if Qr else None, Qr, _ptr(eig), _ptr(z), _ptr(info), _ptr(sets),
                                                  _ptr(fits), _ptr(coef), _ptr(held)))
        return eig, z, info, sets, fits, coef, held

    def spectral_path_times(self):
        """(ms of kernel E1, ms of kernel E2) of the last ``spectral_path`` call (``fsnap_spectral_path_times``)."""
        ms = np.zeros(2)
        self._check(self._lib.fsnap_spectral_path_times(self._h, _ptr(ms)))
        return float(ms[0]), float(ms[1])

    def ard_path(self, d_stats_ptr: int, K: int, F: int, nsub: int, hyper, max_iter: int, tol: float):
        """Grouped K-fold ARD threshold path on per-fold statistics in device memory (``fsnap_ard_path``, K <= 144):
        ``d_stats_ptr`` as for ``lasso_path``; ``hyper`` ((F + 1) x Q x 6: alpha_1, alpha_2, lambda_1, lambda_2,
        threshold_lambda, alpha_init of every problem).  Returns (coef ((F + 1) x Q x K; index F: no fold left out), lambdas
        (the same shape), info ((F + 1) x Q x 6: iterations, kept columns, final alpha_, last sum |coef_old - coef|, smallest
        pivot of the scaled matrices, status 0 converged or emptied / 1 failed / 2 max_iter reached), heldout (F x Q x 3: n_f,
        weighted squared error of fold f under its own refit, bb_f))."""
        hyper = _f64(hyper, "hyper")
        K, F = int(K), int(F)
        if hyper.ndim != 3 or hyper.shape[0] != max(F, 0) + 1 or hyper.shape[2] != 6:
            raise ValueError(f"hyper must have shape (F + 1, Q, 6), not {hyper.shape}")
        Q = hyper.shape[1]
        coef = np.empty((max(F, 0) + 1, Q, max(K, 0)))
        lam = np.empty((max(F, 0) + 1, Q, max(K, 0)))
        info = np.empty((max(F, 0) + 1, Q, 6))
        held = np.empty((max(F, 0), Q, 3))
        self._check(self._lib.fsnap_ard_path(self._h, K, F, int(nsub), c_void_p(d_stats_ptr), _ptr(hyper) if Q else None, Q,
                                             int(max_iter), float(tol), _ptr(coef), _ptr(lam), _ptr(info), _ptr(held)))
        return coef, lam, info, held

    def trsm_pass(self, R, first: bool, d_Q_ptr: int, family: int = 0):
        """One pass Q <- X R^-1 (fsnap_trsm_pass): ``R`` K x K upper triangular on the host; ``first``: X = diag(w_eff) A of
        the resident rows written to the device buffer at ``d_Q_ptr`` (m x K, contiguous), else in place on that buffer;
        ``family`` 0 = the kernel lstsq_rows picks, 1 = kernel 13C, 2 / 3 = kernel 13B with 16- / 32-row tiles.  Returns the
        family that ran."""
        R = _f64(R, "R")
        if R.shape != (self.K, self.K):
            raise ValueError(f"R has shape {R.shape}, expected ({self.K}, {self.K})")
        ran = c_int(0)
        self._check(self._lib.fsnap_trsm_pass(self._h, _ptr(R), int(bool(first)), int(family), c_void_p(d_Q_ptr), byref(ran)))
        return ran.value

    def qpack_device(self, d_qpack_ptr: int):
        """(w_eff != 0, w_eff b) per resident row into the device buffer at ``d_qpack_ptr`` (2 m doubles)."""
        self._check(self._lib.fsnap_qpack_device(self._h, c_void_p(d_qpack_ptr)))

    def lstsq_rows(self, rcond: float, K: int = None):
        """``lstsq(aw, bw, rcond)`` of the resident rows computed on the rows (fsnap_lstsq_rows); collective when the
        context has a communicator.  Returns (beta, rank, info dict)."""
        K = self.K if K is None else int(K)
        beta = np.empty(K, dtype=np.float64)
        rank = c_int(0)
        info = np.zeros(8)
        rc = self._lib.fsnap_lstsq_rows(self._h, float(rcond), K, _ptr(beta), byref(rank), _ptr(info))
        if rc != OK:
            raise_status(rc, (self._lib.fsnap_last_error(self._h) or b"").decode())
        keys = ("passes", "deviation", "converged", "svd", "sigma_max", "sigma_min", "refine_step", "shift")
        return beta, rank.value, dict(zip(keys, info.tolist()))

    # -- multi-GPU (native RCCL) ----------------------------------------------------------
    def comm_init(self, nranks: int, rank: int, ident: bytes):
        if len(ident) != COMM_ID_BYTES:
            raise ValueError("communicator id must be 128 bytes")
        self._check(self._lib.fsnap_comm_init(self._h, int(nranks), int(rank), ctypes.c_char_p(ident)))

    def comm_destroy(self):
        self._check(self._lib.fsnap_comm_destroy(self._h))

    def comm_transport(self) -> str:
        """"none" | "rccl" | "p2p": what this context's communicator runs on."""
        t = c_int(0)
        self._check(self._lib.fsnap_comm_transport(self._h, byref(t)))
        return TRANSPORTS[t.value]

    def comm_info(self):
        n, r = c_int(1), c_int(0)
        self._check(self._lib.fsnap_comm_info(self._h, byref(n), byref(r)))
        return n.value, r.value

    def allreduce_device(self, d_ptr: int, n: int):
        self._check(self._lib.fsnap_allreduce_device(self._h, c_void_p(d_ptr), int(n)))

    def allreduce_host(self, arr: np.ndarray, op: int = REDUCE_SUM):
        """In-place reduction of a C-contiguous float64 array over the ranks."""
        if arr.dtype != np.float64 or not arr.flags["C_CONTIGUOUS"]:
            raise ValueError("allreduce_host needs a C-contiguous float64 array")
        if arr.size:
            self._check(self._lib.fsnap_allreduce_host(self._h, _ptr(arr), arr.size, int(op)))
        return arr

    def bcast_bytes(self, data: bytes, nbytes: int, root: int = 0) -> bytes:
        buf = ctypes.create_string_buffer(data if data is not None else b"", int(nbytes))
        self._check(self._lib.fsnap_bcast_host(self._h, buf, int(nbytes), int(root)))
        return buf.raw

    def allgather_bytes(self, data: bytes, nranks: int) -> list:
        """Equal-size byte strings of all ranks, in rank order."""
        n = len(data)
        out = ctypes.create_string_buffer(n * nranks)
        self._check(self._lib.fsnap_allgather_host(self._h, ctypes.c_char_p(data), n, out))
        raw = out.raw
        return [raw[i * n:(i + 1) * n] for i in range(nranks)]

    def barrier(self):
        self._check(self._lib.fsnap_barrier(self._h))

    def fit_dist(self, kind: int, param: float, K: int):
        """One multi-GPU fit (fsnap_fit_dist): local statistics, in-place RCCL all-reduce, solve on every rank.
        Returns (beta, rank, rcond_estimate, device address of the reduced statistics)."""
        beta = np.empty(int(K), dtype=np.float64)
        rank = c_int(0)
        rce = c_double(0.0)
        ptr = c_void_p()
        rc = self._lib.fsnap_fit_dist(self._h, int(kind), float(param), int(K), _ptr(beta), byref(rank), byref(rce), byref(ptr))
        if rc != OK:
            raise_status(rc, (self._lib.fsnap_last_error(self._h) or b"").decode() if rc < 0 else "")
        return beta, rank.value, rce.value, ptr.value

    # -- raw device memory ----------------------------------------------------------------
    def dev_alloc(self, nbytes: int) -> int:
        ptr = c_void_p()
        self._check(self._lib.fsnap_dev_alloc(self._h, int(nbytes), byref(ptr)))
        return ptr.value

    def dev_free(self, d_ptr: int):
        self._check(self._lib.fsnap_dev_free(self._h, c_void_p(d_ptr)))

    def dev_upload(self, d_ptr: int, arr: np.ndarray):
        arr = np.ascontiguousarray(arr)
        self._check(self._lib.fsnap_dev_upload(self._h, c_void_p(d_ptr), _ptr(arr), arr.nbytes))

    def dev_download(self, d_ptr: int, out: np.ndarray):
        if not out.flags["C_CONTIGUOUS"]:
            raise ValueError("dev_download needs a C-contiguous array")
        self._check(self._lib.fsnap_dev_download(self._h, _ptr(out), c_void_p(d_ptr), out.nbytes))
        return out

    def sync(self):
        self._check(self._lib.fsnap_dev_sync(self._h))

    # -- measurement -------------------------------------------------------------------
    def timing(self, n: int = 8):
        """HIP-event timings (ms); ``n`` = how many leading entries to evaluate (2 = kernels of the last fit only)."""
        ms = (c_double * 8)()
        self._check(self._lib.fsnap_timing(self._h, ms, int(n)))
        return {"syrk_ms": ms[0], "reduce_ms": ms[1], "upload_ms": ms[2], "weight_ms": ms[3], "predict_ms": ms[4],
                "upload_probe_GBps": ms[5], "upload_staged": bool(ms[6])}

    def timing_history(self, n: int):
        """(syrk_ms, reduce_ms) arrays of the last ``n`` fits (oldest first), read from HIP events after the fact."""
        a = np.empty(int(n))
        b = np.empty(int(n))
        self._check(self._lib.fsnap_timing_history(self._h, _ptr(a), _ptr(b), int(n)))
        return a, b

    def timing_history_comm(self, n: int):
        """Collective time (ms) on this rank's stream for the last ``n`` event-bracketed fits, -1 where a fit had none."""
        a = np.empty(int(n))
        self._check(self._lib.fsnap_timing_history_comm(self._h, _ptr(a), int(n)))
        return a

    def timing_count(self):
        """(event-bracketed SYRK launches, all SYRK launches) of this context so far (option ``timing_every``)."""
        a, b = c_int64(0), c_int64(0)
        self._check(self._lib.fsnap_timing_count(self._h, ctypes.byref(a), ctypes.byref(b)))
        return int(a.value), int(b.value)

    def launch_info(self):
        info = (c_int64 * 8)()
        self._check(self._lib.fsnap_launch_info(self._h, info, 8))
        out = {"workgroups": info[0], "threads": info[1], "chunks_per_wave": info[2], "NB": info[3],
               "split": info[4], "compute_units": info[5], "kernel_or_pairs": info[6], "nsplit": info[7]}
        if info[4] != 0:            # not the tiled kernel: the last slot says whether kernel 1A packs its rows' weights itself
            out["nsplit"] = 0
            out["fused_pack"] = info[7]
        return out
