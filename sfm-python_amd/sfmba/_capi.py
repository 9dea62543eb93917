"""ctypes binding of libsfmba.so (include/sfmba.h).  Thin by design: plain pointers and sizes.

There is NO CPU fallback: if the HIP library is missing or no MI355X is visible the calls raise.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SFMBA_LIB") or os.path.join(_HERE, "libsfmba.so")   # SFMBA_LIB: diagnostic builds

class Options(C.Structure):
    _fields_ = [("ftol", C.c_double), ("xtol", C.c_double), ("gtol", C.c_double),
                ("max_nfev", C.c_int64), ("verbose", C.c_int32), ("max_iter", C.c_int32),
                ("pcg_tol", C.c_double), ("pcg_max_iter", C.c_int32), ("pcg_check_every", C.c_int32),
                ("reg_min", C.c_double), ("profile", C.c_int32), ("reserved", C.c_int32),
                ("pcg_tol_max", C.c_double)]


class Result(C.Structure):
    _fields_ = [("cost", C.c_double), ("cost0", C.c_double), ("optimality", C.c_double),
                ("rmse", C.c_double), ("rmse0", C.c_double), ("nfev", C.c_int64), ("njev", C.c_int64),
                ("iterations", C.c_int64), ("pcg_iterations", C.c_int64), ("status", C.c_int32),
                ("reserved", C.c_int32), ("seconds_total", C.c_double), ("seconds_device", C.c_double),
                ("resjac_avg_us", C.c_double), ("resjac_launches", C.c_int64),
                ("last_step_norm", C.c_double), ("last_reg", C.c_double)]


class FilterOptions(C.Structure):
    _fields_ = [("max_error_px", C.c_double), ("min_depth", C.c_double), ("min_angle_deg", C.c_double),
                ("min_views", C.c_int32), ("reserved", C.c_int32)]


class StatsSummary(C.Structure):
    _fields_ = [("n_obs", C.c_int64), ("n_obs_kept", C.c_int64), ("n_points_kept", C.c_int64),
                ("n_behind", C.c_int64), ("sum_err", C.c_double), ("sum_err2", C.c_double), ("max_err", C.c_double)]


class TriangulateOptions(C.Structure):
    _fields_ = [("max_iter", C.c_int32), ("min_views", C.c_int32), ("xtol", C.c_double), ("min_angle_deg", C.c_double),
                ("min_depth", C.c_double), ("max_error_px", C.c_double)]


class ResectOptions(C.Structure):
    _fields_ = [("max_iter", C.c_int32), ("min_views", C.c_int32), ("start", C.c_int32), ("xtol", C.c_double),
                ("min_depth", C.c_double), ("max_rms_px", C.c_double)]


class PnpRansacOptions(C.Structure):
    _fields_ = [("threshold", C.c_double), ("confidence", C.c_double), ("min_depth", C.c_double), ("seed", C.c_uint64),
                ("max_iters", C.c_int32), ("min_views", C.c_int32), ("refine", C.c_int32), ("profile", C.c_int32),
                ("max_iter", C.c_int32), ("reserved", C.c_int32), ("xtol", C.c_double), ("max_rms_px", C.c_double)]


class TriRansacOptions(C.Structure):
    _fields_ = [("threshold", C.c_double), ("min_depth", C.c_double), ("min_pair_angle_deg", C.c_double), ("seed", C.c_uint64),
                ("max_pairs", C.c_int32), ("min_views", C.c_int32), ("refine", C.c_int32), ("profile", C.c_int32),
                ("max_iter", C.c_int32), ("reserved", C.c_int32), ("xtol", C.c_double), ("min_angle_deg", C.c_double),
                ("max_error_px", C.c_double)]


class RansacOptions(C.Structure):
    _fields_ = [("threshold", C.c_double), ("confidence", C.c_double), ("seed", C.c_uint64), ("max_iters", C.c_int32),
                ("refit", C.c_int32), ("profile", C.c_int32), ("reserved", C.c_int32)]


class PoseOptions(C.Structure):
    _fields_ = [("min_depth", C.c_double), ("profile", C.c_int32), ("reserved", C.c_int32)]


class MatchOptions(C.Structure):
    _fields_ = [("ratio", C.c_double), ("form", C.c_int32), ("profile", C.c_int32)]


class TrackOptions(C.Structure):
    _fields_ = [("min_length", C.c_int32), ("max_length", C.c_int32), ("conflicts", C.c_int32), ("profile", C.c_int32)]


class PlanOptions(C.Structure):
    _fields_ = [("min_views", C.c_int32), ("profile", C.c_int32)]


class CovarianceOptions(C.Structure):
    _fields_ = [("kind", C.c_int32), ("gauge", C.c_int32), ("sigma2", C.c_double), ("rank_tol", C.c_double),
                ("point_tol", C.c_double), ("profile", C.c_int32), ("reserved", C.c_int32)]


class CovarianceInfo(C.Structure):
    _fields_ = [("status", C.c_int32), ("g0", C.c_int32), ("g1", C.c_int32), ("g1_axis", C.c_int32), ("n_free", C.c_int32),
                ("n_held", C.c_int32), ("bad_param", C.c_int32), ("reserved", C.c_int32), ("dof", C.c_int64),
                ("n_bad_points", C.c_int64), ("bad_point", C.c_int64), ("sigma2", C.c_double), ("cost", C.c_double),
                ("min_pivot_rel", C.c_double), ("kernel_us", C.c_double)]


ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32)
PRINT_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_char_p)

P, INT, I32, I64, F64, STR, REF = C.c_void_p, C.c_int, C.c_int32, C.c_int64, C.c_double, C.c_char_p, C.POINTER

# Every function include/sfmba.h declares, in its order: name -> (restype, argtypes).  P is any data pointer, REF(S) a
# pointer to an option, result or info structure or to a scalar passed with byref.  tests/test_host_cabi.py holds every
# entry, and every structure above, to the header.
SIGNATURES = {
    "sfmba_create": (INT, [REF(P), INT]),
    "sfmba_destroy": (None, [P]),
    "sfmba_last_error": (STR, [P]),
    "sfmba_default_options": (None, [REF(Options)]),
    "sfmba_set_print": (INT, [P, PRINT_FN, P]),
    "sfmba_set_stream": (INT, [P, P]),
    "sfmba_set_precision": (INT, [P, I32]),
    "sfmba_set_problem": (INT, [P, I64, I64, I64, P, P, P, P]),
    "sfmba_problem_reuse": (INT, [P, REF(I64), REF(I64)]),
    "sfmba_set_problem_i64": (INT, [P, I64, I64, I64, P, P, P, P]),
    "sfmba_set_fixed_cameras": (INT, [P, P, I64]),
    "sfmba_exchange_doubles": (I64, [I64]),
    "sfmba_set_exchange": (INT, [P, P, I64, ALLREDUCE_FN, P, I64]),
    "sfmba_comm_get_unique_id": (INT, [P]),
    "sfmba_comm_init": (INT, [P, P, I32, I32, I64]),
    "sfmba_comm_destroy": (INT, [P]),
    "sfmba_p2p_export": (INT, [P, I32, P]),
    "sfmba_p2p_attach": (INT, [P, P, I32, I32]),
    "sfmba_p2p_detach": (INT, [P]),
    "sfmba_p2p_calls": (I64, [P]),
    "sfmba_get_counters": (INT, [P, REF(I64), REF(I64)]),
    "sfmba_get_form": (INT, [P, STR, REF(I32)]),
    "sfmba_get_pcg_history": (I32, [P, P, I32]),
    "sfmba_residuals": (INT, [P, P, P]),
    "sfmba_residual_jacobian": (INT, [P, P, P, P, P]),
    "sfmba_default_filter_options": (None, [REF(FilterOptions)]),
    "sfmba_reprojection_stats": (INT, [P, P, REF(FilterOptions)] + [P] * 13 + [REF(StatsSummary)]),
    "sfmba_default_triangulate_options": (None, [REF(TriangulateOptions)]),
    "sfmba_triangulate": (INT, [P, P, P, P, REF(TriangulateOptions)] + [P] * 6 + [REF(I64)]),
    "sfmba_default_resect_options": (None, [REF(ResectOptions)]),
    "sfmba_resect": (INT, [P, P, P, P, REF(ResectOptions)] + [P] * 5 + [REF(I64)]),
    "sfmba_default_pnp_ransac_options": (None, [REF(PnpRansacOptions)]),
    "sfmba_resect_ransac": (INT, [P] * 5 + [REF(PnpRansacOptions)] + [P] * 12 + [REF(I64), REF(F64)]),
    "sfmba_default_tri_ransac_options": (None, [REF(TriRansacOptions)]),
    "sfmba_triangulate_ransac": (INT, [P] * 4 + [REF(TriRansacOptions)] + [P] * 11 + [REF(I64), REF(F64)]),
    "sfmba_default_ransac_options": (None, [REF(RansacOptions)]),
    "sfmba_fundamental_ransac": (INT, [P, I64] + [P] * 5 + [REF(RansacOptions)] + [P] * 8 + [REF(I64), REF(F64)]),
    "sfmba_homography_ransac": (INT, [P, I64] + [P] * 5 + [REF(RansacOptions)] + [P] * 10 + [REF(I64), REF(F64)]),
    "sfmba_similarity_ransac": (INT, [P, I64] + [P] * 5 + [REF(RansacOptions)] + [P] * 10 + [REF(I64), REF(F64)]),
    "sfmba_essential_ransac": (INT, [P, I64] + [P] * 6 + [REF(RansacOptions)] + [P] * 9 + [REF(I64), REF(F64)]),
    "sfmba_default_pose_options": (None, [REF(PoseOptions)]),
    "sfmba_recover_pose": (INT, [P, I64] + [P] * 6 + [REF(PoseOptions)] + [P] * 9 + [REF(I64), REF(F64)]),
    "sfmba_set_descriptors": (INT, [P, I64, P, P, I32, I32, REF(I32)]),
    "sfmba_default_match_options": (None, [REF(MatchOptions)]),
    "sfmba_match_descriptors": (INT, [P, I64, P, REF(MatchOptions)] + [P] * 6 + [REF(I64), REF(F64)]),
    "sfmba_default_track_options": (None, [REF(TrackOptions)]),
    "sfmba_build_tracks": (INT, [P, I64, P, I64, P, P, P, P, REF(TrackOptions), P, P, REF(F64)]),
    "sfmba_get_tracks": (INT, [P, P, P, P]),
    "sfmba_default_plan_options": (None, [REF(PlanOptions)]),
    "sfmba_set_keypoints": (INT, [P, I64, P, P]),
    "sfmba_plan_views": (INT, [P, I64, P, I64, P, REF(PlanOptions)] + [P] * 5 + [REF(F64)]),
    "sfmba_assemble_problem": (INT, [P, I64, P, I64, P, REF(PlanOptions), P, REF(F64)]),
    "sfmba_get_assembled": (INT, [P] * 7),
    "sfmba_solve": (INT, [P, P, REF(Options), REF(Result)]),
    "sfmba_solve_from": (INT, [P, P, P, REF(Options), REF(Result)]),
    "sfmba_get_fun_grad": (INT, [P, P, P]),
    "sfmba_default_covariance_options": (None, [REF(CovarianceOptions)]),
    "sfmba_covariance": (INT, [P, P, P, I32, REF(CovarianceOptions)] + [P] * 7 + [REF(CovarianceInfo)]),
    "sfmba_time_kernel": (INT, [P, P, I32, I32, REF(F64)]),
    "sfmba_normal_blocks": (INT, [P] * 6),
    "sfmba_schur_matvec": (INT, [P] * 6),
    "sfmba_step_products": (INT, [P] * 11),
    "sfmba_rhs_precond": (INT, [P] * 7),
    "sfmba_get_mixed_operands": (INT, [P] * 5),
    "sfmba_get_iteration_state": (INT, [P] * 17),
    "sfmba_dense_schur": (INT, [P] * 7),
    "sfmba_tr2d_solve": (INT, [P, P, F64, P]),
    "sfmba_debug_option": (INT, [P, STR, I64]),
}
SYMBOLS = tuple(SIGNATURES)     # (tests check the library exports each of them)

_lib = None


def _share_hip_runtime_with_torch():
    """One HIP runtime per process.  libsfmba.so needs `libamdhip64.so.7`; a PyTorch-ROCm wheel ships its own copy of that
    library (and of the HSA runtime) under torch/lib and loads it by path.  Whichever is loaded first wins the SONAME, and
    when the system's copy came first, `torch.cuda` later finds "No HIP GPUs" in this process (seen on this image: ROCm 7.2
    under /opt/rocm, 7.0 inside the wheel).  The package works with torch at its side (streams handed over by
    `set_stream`, `sfmba.dist`), so when torch is INSTALLED -- imported or not -- its copy is loaded first, and
    libsfmba.so binds to it exactly as it does when `import torch` came first.  SFMBA_HIP_RUNTIME=system skips this."""
    if os.environ.get("SFMBA_HIP_RUNTIME", "") == "system":
        return
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return                                             # torch's libraries are in the process already
    try:
        spec = importlib.util.find_spec("torch")           # (locates the package without importing it)
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    libdir = os.path.join(os.path.dirname(spec.origin), "lib")
    for name in ("libhsa-runtime64.so", "libamdhip64.so"):
        path = os.path.join(libdir, name)
        if os.path.exists(path):
            try:
                C.CDLL(path, mode=C.RTLD_GLOBAL)
            except OSError:
                return


def load():
    """Load libsfmba.so (raises if it has not been built: there is no fallback path)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: build the HIP back end first (python __graft_entry__.py, or "
            "make -C sfm-python_amd).  sfmba has no CPU fallback.")
    _share_hip_runtime_with_torch()
    lib = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in SIGNATURES.items():
        if hasattr(lib, name):      # (an older build given through SFMBA_LIB for an A/B run lacks the newer functions)
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, argtypes
    _lib = lib
    return lib


def ptr(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)
