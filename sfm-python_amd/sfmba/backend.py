"""Handle wrapper around the C-ABI: owns one sfmba_handle (one GPU, one problem at a time)."""
from __future__ import annotations

import ctypes as C
import weakref

import numpy as np

from . import _capi
from .checks import (_edge_batch, _f64, _fill_options, _mask, _opt_ptr, _ransac_prologue,  # noqa: F401 (imported from here too)
                     check_descriptors, check_essential_args, check_match_edges, check_match_options, check_plan_inputs,
                     check_similarity_inputs, check_track_inputs)
from .results import (Covariance, DescriptorMatches, EssentialEstimate, FundamentalEstimate,  # noqa: F401 (likewise)
                      HomographyEstimate, RelativePose, ReprojectionStats, Resection, RobustResection, RobustTriangulation,
                      SimilarityEstimate, SubProblem, Tracks, Triangulation, ViewPlan)


class BackendError(RuntimeError):
    pass


# The pair-RANSAC models as `Backend._pair_ransac` needs them (csrc/consumers.hip: TwoViewRansac).  ``S`` pairs make a
# sample; ``models`` are the (E, *shape) float64 outputs, ``masks`` the (M) ones, ``cols`` the int32 (E) columns ahead of
# ``success`` and ``status``, ``hyps`` the optional (E, H) ones, each in the order of the C call; ``strict`` is the mode of
# `_ransac_prologue`.  A batch of ``set``s has 3-D points and its own argument names; ``nan_options``: a NaN threshold or
# confidence is refused here, in the words of `check_similarity_inputs`, not by the library; ``calibrated``: the call takes K.
_FUNDAMENTAL = dict(fn="sfmba_fundamental_ransac", S=8, strict=False, models=("F", "F_refit"), shape=(3, 3),
                    masks=("inlier_mask",), cols=("inliers", "best"), hyps=("hyp_inliers",))
_HOMOGRAPHY = dict(fn="sfmba_homography_ransac", S=4, strict=True, models=("H", "H_refit"), shape=(3, 3),
                   masks=("inlier_mask", "refit_mask"), cols=("inliers", "refit_inliers", "best"), hyps=("hyp_inliers",))
_SIMILARITY = dict(fn="sfmba_similarity_ransac", S=3, strict=False, models=("sim", "sim_refit"), shape=(13,),
                   masks=("inlier_mask", "refit_mask"), cols=("inliers", "refit_inliers", "best"), hyps=("hyp_inliers",),
                   batch="set", dim=3, names=("src", "dst", "set_ptr"), what="similarity RANSAC", nan_options=True)
_ESSENTIAL = dict(fn="sfmba_essential_ransac", S=5, strict=True, models=("E",), shape=(3, 3),
                  masks=("inlier_mask",), cols=("inliers", "best", "best_root"), hyps=("hyp_inliers", "hyp_roots"), calibrated=True)


class Backend:
    """One MI355X.  Not thread-safe; use one Backend per thread (include/sfmba.h, Threading)."""

    def __init__(self, device: int = 0):
        self._lib = _capi.load()
        self._h = C.c_void_p()
        rc = self._lib.sfmba_create(C.byref(self._h), int(device))
        if rc != 0:
            self._h = None
            raise BackendError(
                f"sfmba_create(device={device}) failed with code {rc}: no usable MI355X/HIP device. "
                "The bundle-adjustment path has no CPU fallback.")
        self.device = int(device)
        self.n_cameras = self.n_points = self.n_obs = 0
        self._keep = []          # arrays / callbacks the library borrows beyond one call
        # the verbose = 2 iteration table goes through Python's sys.stdout, like scipy's print() calls
        # (looked up at call time, so contextlib.redirect_stdout and notebook capture see it)
        self._print_cb = _capi.PRINT_FN(lambda ctx, line: print(line.decode("utf-8", "replace")))
        self._lib.sfmba_set_print(self._h, self._print_cb, None)

    def close(self):
        if getattr(self, "_h", None):
            try:
                self._flush_pending()
            except Exception:                                  # noqa: BLE001 (a dying handle must still be released)
                pass
            self._lib.sfmba_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------------------------------
    def _check(self, rc: int):
        if rc == 0:
            return
        msg = self._lib.sfmba_last_error(self._h).decode("utf-8", "replace")
        if rc in (-1, -2):
            raise ValueError(msg)            # scipy raises ValueError for both (least_squares.py:844)
        if rc == -4:
            raise MemoryError(msg)
        raise BackendError(f"sfmba error {rc}: {msg}")

    # ---- results left on the device -----------------------------------------------------------------
    # The reference reads only ``result.x`` (sfm.py:271,281), and ``result.fun`` is 16 MB at a million observations:
    # `solve(..., want_fun=False, want_grad=False)` leaves fun and grad in the handle's buffers and registers the result object (weakly).  They are
    # downloaded when somebody looks at them, or -- if the object is still alive -- right before this handle's next
    # operation overwrites the buffers; a result that was dropped unread costs no download at all.
    def _flush_pending(self):
        ref, self._pending = getattr(self, "_pending", None), None
        if ref is not None:
            obj = ref()
            if obj is not None:
                obj._materialize()

    def _register_pending(self, obj):
        self._pending = weakref.ref(obj)

    def fetch_fun_grad(self, want_fun=True, want_grad=True):
        """fun (2 n_obs) and / or grad (n) of the last solve, while the handle still holds them."""
        fun = np.empty(2 * self.n_obs) if want_fun else None
        grad = np.empty(self.n_params) if want_grad else None
        if want_fun or want_grad:
            self._check(self._lib.sfmba_get_fun_grad(self._h, _capi.ptr(fun) if want_fun else None,
                                                     _capi.ptr(grad) if want_grad else None))
        return fun, grad

    def set_precision(self, storage_bits: int):
        """64 (default) or 32: storage of uv / r / Jacobian; arithmetic stays fp64.  Applies from the
        next set_problem."""
        self._flush_pending()
        self._check(self._lib.sfmba_set_precision(self._h, int(storage_bits)))

    def set_fixed_cameras(self, camera_indices=()):
        """Cameras whose six parameters stay as they are (``create_sparsity_matrix(..., fixed_camera_indices)``).
        Applies from the next set_problem until replaced."""
        idx = np.ascontiguousarray(sorted(set(int(c) for c in camera_indices)), dtype=np.int64)
        if tuple(idx) == getattr(self, "_fixed", ()):
            return
        self._flush_pending()
        self._check(self._lib.sfmba_set_fixed_cameras(self._h, _capi.ptr(idx) if len(idx) else None, len(idx)))
        self._fixed = tuple(int(c) for c in idx)

    def debug_option(self, name: str, value: int):
        """Test / diagnostic hook (include/sfmba.h: sfmba_debug_option)."""
        self._check(self._lib.sfmba_debug_option(self._h, name.encode(), int(value)))

    def set_stream(self, hip_stream: int):
        self._check(self._lib.sfmba_set_stream(self._h, C.c_void_p(int(hip_stream))))

    def set_problem(self, n_cameras, n_points, camera_indices, point_indices, points_2d, K):
        self._flush_pending()
        ci = np.ascontiguousarray(camera_indices, dtype=np.int64).ravel()
        pi = np.ascontiguousarray(point_indices, dtype=np.int64).ravel()
        if ci.shape != pi.shape:
            raise ValueError("camera_indices and point_indices differ in length")
        n_obs = ci.shape[0]
        Kc = _f64(K, (3, 3), "K")
        p2 = np.asarray(points_2d)
        if p2.dtype == np.int64 and p2.shape == (n_obs, 2) and p2.flags.c_contiguous:
            # the reference's own pixel arrays (graph.py:112-113): handed over as they are
            self._check(self._lib.sfmba_set_problem_i64(self._h, int(n_cameras), int(n_points), n_obs,
                                                        _capi.ptr(ci), _capi.ptr(pi), _capi.ptr(p2),
                                                        _capi.ptr(Kc)))
        else:
            uv = _f64(points_2d, (n_obs, 2), "points_2d")    # promoted as bundle_adjustment.py:41
            self._check(self._lib.sfmba_set_problem(self._h, int(n_cameras), int(n_points), n_obs,
                                                    _capi.ptr(ci), _capi.ptr(pi), _capi.ptr(uv),
                                                    _capi.ptr(Kc)))
        self.n_cameras, self.n_points, self.n_obs = int(n_cameras), int(n_points), n_obs
        self._keep = []

    @property
    def n_params(self):
        return 6 * self.n_cameras + 3 * self.n_points

    def exchange_doubles(self) -> int:
        return int(self._lib.sfmba_exchange_doubles(self.n_cameras))

    def set_exchange(self, arena_ptr: int, arena_doubles: int, callback, n_obs_total: int):
        """callback(dev_ptr:int, count:int, op:int) -> None; op 0 sum, 1 max."""
        if callback is None:
            self._check(self._lib.sfmba_set_exchange(self._h, None, 0, _capi.ALLREDUCE_FN(), None, 0))
            self._keep = []
            return

        def _tramp(ctx, dev_ptr, count, op):
            try:
                callback(int(dev_ptr), int(count), int(op))
                return 0
            except Exception as exc:                         # noqa: BLE001 -- reported through rc
                import traceback
                traceback.print_exc()
                self._cb_error = exc
                return 1

        cfn = _capi.ALLREDUCE_FN(_tramp)
        self._keep = [cfn, callback]
        self._check(self._lib.sfmba_set_exchange(self._h, C.c_void_p(int(arena_ptr)),
                                                 int(arena_doubles), cfn, None, int(n_obs_total)))

    @staticmethod
    def comm_unique_id() -> bytes:
        """128-byte RCCL id; call on rank 0 and broadcast (sfmba.dist.NativeComm does)."""
        buf = C.create_string_buffer(128)
        rc = _capi.load().sfmba_comm_get_unique_id(buf)
        if rc != 0:
            raise BackendError("sfmba_comm_get_unique_id failed: librccl.so.1 not loadable")
        return buf.raw

    def comm_init(self, unique_id: bytes, rank: int, world: int, n_obs_total: int):
        if len(unique_id) != 128:
            raise ValueError("unique_id must be 128 bytes")
        buf = C.create_string_buffer(unique_id, 128)
        self._check(self._lib.sfmba_comm_init(self._h, buf, int(rank), int(world), int(n_obs_total)))

    def comm_destroy(self):
        self._check(self._lib.sfmba_comm_destroy(self._h))

    # direct all-reduce over peer-mapped memory (include/sfmba.h: sfmba_p2p_*)
    def p2p_export(self, world: int) -> bytes:
        buf = C.create_string_buffer(64)
        self._check(self._lib.sfmba_p2p_export(self._h, int(world), buf))
        return buf.raw

    def p2p_attach(self, handles: bytes, rank: int, world: int) -> int:
        """Returns the C-ABI code (0 attached, -5 mapping or self-test failed) instead of raising: the
        caller has to agree on the outcome with the other ranks first."""
        if len(handles) != 64 * world:
            raise ValueError("handles must hold world x 64 bytes")
        buf = C.create_string_buffer(handles, len(handles))
        return int(self._lib.sfmba_p2p_attach(self._h, buf, int(rank), int(world)))

    def p2p_detach(self):
        self._check(self._lib.sfmba_p2p_detach(self._h))

    def problem_reuse(self):
        """(observations re-used from the previous problem of this handle, observations uploaded) of the last
        set_problem (include/sfmba.h: incremental re-use)."""
        a, b = C.c_int64(), C.c_int64()
        self._lib.sfmba_problem_reuse(self._h, C.byref(a), C.byref(b))
        return int(a.value), int(b.value)

    def counters(self):
        """(kernel launches, collectives) enqueued by this handle so far."""
        a, b = C.c_int64(), C.c_int64()
        self._lib.sfmba_get_counters(self._h, C.byref(a), C.byref(b))
        return int(a.value), int(b.value)

    def form(self, name: str) -> int:
        """Whether the current problem runs the named kernel form (include/sfmba.h: sfmba_get_form)."""
        v = C.c_int32()
        self._check(self._lib.sfmba_get_form(self._h, name.encode(), C.byref(v)))
        return int(v.value)

    def pcg_history(self):
        """PCG iterations of every outer iteration of the last solve on this handle."""
        n = int(self._lib.sfmba_get_pcg_history(self._h, None, 0))        # (returns the count, writes min(count, cap))
        buf = (C.c_int32 * max(n, 1))()
        n = min(n, int(self._lib.sfmba_get_pcg_history(self._h, buf, n)))
        return [int(buf[k]) for k in range(n)]

    def p2p_calls(self) -> int:
        return int(self._lib.sfmba_p2p_calls(self._h))

    # ------------------------------------------------------------------------------------------
    def residuals(self, x):
        self._flush_pending()
        x = _f64(x, (self.n_params,), "x")
        out = np.empty(2 * self.n_obs)
        self._check(self._lib.sfmba_residuals(self._h, _capi.ptr(x), _capi.ptr(out)))
        return out

    def reprojection_stats(self, x, max_error_px=np.inf, min_depth=-np.inf, min_angle_deg=0.0, min_views=0,
                           want=("obs", "points", "cameras")):
        """Reprojection error, depth and keep mask per observation, track statistics per point, error statistics per
        camera and a summary at ``x``, in one sweep on the device (include/sfmba.h: sfmba_reprojection_stats).  An
        observation is kept when ``err <= max_error_px`` and ``depth > min_depth`` and its point is kept; a point when
        it has ``min_views`` such observations and their rays open at least ``min_angle_deg``.  The defaults keep
        everything.  ``want``: which groups of arrays to download ("obs", "points", "cameras"); the summary always comes.
        -> :class:`ReprojectionStats`."""
        self._flush_pending()
        x = _f64(x, (self.n_params,), "x")
        want = (want,) if isinstance(want, str) else tuple(want)
        unknown = set(want) - {"obs", "points", "cameras"}
        if unknown:
            raise ValueError(f"unknown group(s) in `want`: {sorted(unknown)}")
        opt = _capi.FilterOptions()
        self._lib.sfmba_default_filter_options(C.byref(opt))
        opt.max_error_px, opt.min_depth, opt.min_angle_deg = float(max_error_px), float(min_depth), float(min_angle_deg)
        opt.min_views = int(min_views)
        N, P, Cn = self.n_obs, self.n_points, self.n_cameras
        spec = (("obs", "obs_err", N, np.float64), ("obs", "obs_depth", N, np.float64), ("obs", "obs_keep", N, np.uint8),
                ("points", "pt_views", P, np.int32), ("points", "pt_max_err", P, np.float64),
                ("points", "pt_sum_err2", P, np.float64), ("points", "pt_min_depth", P, np.float64),
                ("points", "pt_max_angle_deg", P, np.float64), ("points", "pt_keep", P, np.uint8),
                ("cameras", "cam_views", Cn, np.int32), ("cameras", "cam_sum_err", Cn, np.float64),
                ("cameras", "cam_max_err", Cn, np.float64), ("cameras", "cam_behind", Cn, np.int32))
        arrays = {name: np.empty(n, dtype=dt) for group, name, n, dt in spec if group in want}
        ptrs = [_capi.ptr(arrays[name]) if name in arrays else None for _, name, _, _ in spec]
        summary = _capi.StatsSummary()
        self._check(self._lib.sfmba_reprojection_stats(self._h, _capi.ptr(x), C.byref(opt), *ptrs, C.byref(summary)))
        for name in ("obs_keep", "pt_keep"):
            if name in arrays:
                arrays[name] = arrays[name].view(np.bool_)
        return ReprojectionStats(arrays, summary)

    def covariance(self, x, hold=None, kind="marginal", gauge="auto", sigma2=None, want_full=False, want_points=True,
                   **options):
        """Covariance blocks of the solution ``x`` of the current problem (include/sfmba.h: sfmba_covariance).  ``kind``:
        "marginal" (sigma^2 S^-1 and the point blocks that go with it; at most 21 cameras) or "conditional" (each block with
        everything else held; any size).  ``hold``: camera parameters to hold, as indices 6 c + k or (camera, component)
        pairs; ``gauge``: "auto" holds the first camera and one baseline coordinate when nothing else fixes the gauge,
        "none" adds nothing.  ``sigma2`` None: sum r^2 / dof.  ``options``: rank_tol, point_tol, profile.
        -> :class:`Covariance`."""
        self._flush_pending()
        x = _f64(x, (self.n_params,), "x")
        kinds, gauges = {"marginal": 0, "conditional": 1, 0: 0, 1: 1}, {"auto": 1, "none": 0, True: 1, False: 0, None: 0}
        if kind not in kinds or gauge not in gauges:
            raise ValueError("kind is 'marginal' or 'conditional', gauge is 'auto' or 'none'")
        opt = _capi.CovarianceOptions()
        self._lib.sfmba_default_covariance_options(C.byref(opt))
        _fill_options(opt, options, "covariance")
        opt.kind, opt.gauge, opt.sigma2 = kinds[kind], gauges[gauge], 0.0 if sigma2 is None else float(sigma2)
        hold_idx = []
        for q in (() if hold is None else hold):
            hold_idx.append(6 * int(q[0]) + int(q[1]) if np.ndim(q) else int(q))
        hold_arr = np.ascontiguousarray(hold_idx, dtype=np.int32)
        Cn, P = self.n_cameras, self.n_points
        arrays = {"cam_cov": np.empty((Cn, 6, 6)), "cam_sigma": np.empty((Cn, 2)), "pt_status": np.empty(P, dtype=np.int32),
                  "held": np.empty(6 * Cn, dtype=np.uint8)}
        if want_full:
            arrays["cam_full"] = np.empty((6 * Cn, 6 * Cn))
        if want_points:
            arrays["pt_cov"], arrays["pt_sigma"] = np.empty((P, 3, 3)), np.empty(P)
        info = _capi.CovarianceInfo()
        ptrs = [_capi.ptr(arrays[k]) if k in arrays else None
                for k in ("cam_cov", "cam_full", "cam_sigma", "pt_cov", "pt_sigma", "pt_status", "held")]
        self._check(self._lib.sfmba_covariance(self._h, _capi.ptr(x), _capi.ptr(hold_arr) if len(hold_arr) else None,
                                               len(hold_arr), C.byref(opt), *ptrs, C.byref(info)))
        return Covariance(arrays, info)

    def triangulate(self, x, select=None, obs_use=None, **options):
        """Triangulate the selected points of the current problem from their used observations and the cameras of ``x``:
        n-view DLT, then Gauss-Newton on the reprojection error, then a verdict per point (include/sfmba.h:
        sfmba_triangulate).  ``select`` (P) and ``obs_use`` (N, the caller's observation order): boolean masks, None = all.
        ``options``: fields of ``sfmba_triangulate_options`` (max_iter, min_views, xtol, min_angle_deg, min_depth,
        max_error_px).  -> :class:`Triangulation`."""
        self._flush_pending()
        x = _f64(x, (self.n_params,), "x")
        opt = _capi.TriangulateOptions()
        self._lib.sfmba_default_triangulate_options(C.byref(opt))
        _fill_options(opt, options, "triangulation")
        P = self.n_points
        sel, use = _mask(select, P, "select"), _mask(obs_use, self.n_obs, "obs_use")
        points = np.empty((P, 3))
        status, views, iters = (np.empty(P, dtype=np.int32) for _ in range(3))
        rms, ang = np.empty(P), np.empty(P)
        n_ok = C.c_int64()
        self._check(self._lib.sfmba_triangulate(
            self._h, _capi.ptr(x), _capi.ptr(sel) if sel is not None else None,
            _capi.ptr(use) if use is not None else None, C.byref(opt), _capi.ptr(points), _capi.ptr(status),
            _capi.ptr(views), _capi.ptr(iters), _capi.ptr(rms), _capi.ptr(ang), C.byref(n_ok)))
        return Triangulation(points, status, views, iters, rms, ang, n_ok.value)

    def triangulate_ransac(self, x, select=None, obs_use=None, want_hyp=False, **options):
        """Triangulate the selected points of the current problem robustly: hypotheses from pairs of a point's used
        observations (all pairs while there are at most ``max_pairs``, else that many drawn on the device from ``seed``),
        scored over all of them, then :meth:`triangulate` over the inliers of the best (include/sfmba.h:
        sfmba_triangulate_ransac).  ``select`` (P) and ``obs_use`` (N, the caller's order): boolean masks, None = all.
        ``options``: fields of ``sfmba_tri_ransac_options`` (threshold, min_depth, min_pair_angle_deg, seed, max_pairs,
        min_views, refine, profile, max_iter, xtol, min_angle_deg, max_error_px).  ``want_hyp``: also return the count of
        every hypothesis.  -> :class:`RobustTriangulation`."""
        self._flush_pending()
        x = _f64(x, (self.n_params,), "x")
        opt = _capi.TriRansacOptions()
        self._lib.sfmba_default_tri_ransac_options(C.byref(opt))
        options = dict(options)
        if "seed" in options:
            seed = int(options.pop("seed"))
            if not 0 <= seed < 2 ** 64:
                raise ValueError("seed must fit 64 unsigned bits")
            opt.seed = seed
        _fill_options(opt, options, "robust triangulation")
        if opt.max_pairs < 1:
            raise ValueError("max_pairs must be at least 1")
        P, N, H = self.n_points, self.n_obs, int(opt.max_pairs)
        if want_hyp and P * H >= 2 ** 31:
            raise ValueError(f"hyp_inliers of {P} points x {H} pairs passes 2^31 entries")
        sel, use = _mask(select, P, "select"), _mask(obs_use, N, "obs_use")
        points, hyp_points = np.empty((P, 3)), np.empty((P, 3))
        mask = np.zeros(N, dtype=np.uint8)
        status, views, inl, best, iters = (np.empty(P, dtype=np.int32) for _ in range(5))
        rms, ang = np.empty(P), np.empty(P)
        hyp = np.empty((P, H), dtype=np.int32) if want_hyp else None
        n_ok, us = C.c_int64(), C.c_double()
        self._check(self._lib.sfmba_triangulate_ransac(
            self._h, _capi.ptr(x), _opt_ptr(sel), _opt_ptr(use), C.byref(opt), _capi.ptr(points), _capi.ptr(hyp_points),
            _capi.ptr(mask), _capi.ptr(status), _capi.ptr(views), _capi.ptr(inl), _capi.ptr(best), _capi.ptr(iters),
            _capi.ptr(rms), _capi.ptr(ang), _opt_ptr(hyp), C.byref(n_ok), C.byref(us)))
        return RobustTriangulation(points, status, views, iters, rms, ang, int(n_ok.value), hyp_points,
                                   mask.view(np.bool_), inl, best, hyp, float(us.value))

    def resect(self, x, select=None, obs_use=None, **options):
        """Resect the selected cameras of the current problem from their used observations and the points of ``x``:
        n-point DLT (or, ``start=1``, the camera's pose in ``x``), then Gauss-Newton on the reprojection error over the
        six pose parameters, then a verdict per camera (include/sfmba.h: sfmba_resect).  ``select`` (C) and ``obs_use``
        (N, the caller's observation order): boolean masks, None = all.  ``options``: fields of ``sfmba_resect_options``
        (max_iter, min_views, start, xtol, min_depth, max_rms_px).  -> :class:`Resection`."""
        self._flush_pending()
        x = _f64(x, (self.n_params,), "x")
        opt = _capi.ResectOptions()
        self._lib.sfmba_default_resect_options(C.byref(opt))
        _fill_options(opt, options, "resection")
        Cn = self.n_cameras
        sel, use = _mask(select, Cn, "select"), _mask(obs_use, self.n_obs, "obs_use")
        cameras = np.empty((Cn, 6))
        status, views, iters = (np.empty(Cn, dtype=np.int32) for _ in range(3))
        rms = np.empty(Cn)
        n_ok = C.c_int64()
        self._check(self._lib.sfmba_resect(
            self._h, _capi.ptr(x), _capi.ptr(sel) if sel is not None else None,
            _capi.ptr(use) if use is not None else None, C.byref(opt), _capi.ptr(cameras), _capi.ptr(status),
            _capi.ptr(views), _capi.ptr(iters), _capi.ptr(rms), C.byref(n_ok)))
        return Resection(cameras, status, views, iters, rms, n_ok.value)

    def resect_ransac(self, x, select=None, obs_use=None, samples=None, want_hyp=False, **options):
        """Resect the selected cameras of the current problem robustly: ``max_iters`` P3P hypotheses per camera from three
        of its used observations each, scored over all of them, then the refinement of :meth:`resect` over the inliers
        of the best (include/sfmba.h: sfmba_resect_ransac).  ``select`` (C) and ``obs_use`` (N, the caller's order):
        boolean masks, None = all; ``samples`` (C, H, 3) int32 positions among a camera's used observations (camera-major
        stored order), None = drawn on the device from ``seed``.  ``options``: fields of ``sfmba_pnp_ransac_options``
        (threshold, confidence, min_depth, seed, max_iters, min_views, refine, profile, max_iter, xtol, max_rms_px); with
        ``samples`` given, ``max_iters`` defaults to its H.  ``want_hyp``: also return the count of every hypothesis.
        -> :class:`RobustResection`."""
        self._flush_pending()
        x = _f64(x, (self.n_params,), "x")
        opt = _capi.PnpRansacOptions()
        self._lib.sfmba_default_pnp_ransac_options(C.byref(opt))
        Cn, N = self.n_cameras, self.n_obs
        samples = _ransac_prologue(opt, options, samples, Cn, 3, "n_cameras", "camera", "robust resection")
        H = int(opt.max_iters)
        sel, use = _mask(select, Cn, "select"), _mask(obs_use, N, "obs_use")
        cameras, hyp_pose = np.empty((Cn, 6)), np.empty((Cn, 6))
        mask = np.zeros(N, dtype=np.uint8)
        status, views, inl, best, sol, iters = (np.empty(Cn, dtype=np.int32) for _ in range(6))
        success = np.zeros(Cn, dtype=np.uint8)
        rms = np.empty(Cn)
        hyp = np.empty((Cn, H), dtype=np.int32) if want_hyp else None
        n_ok, us = C.c_int64(), C.c_double()
        self._check(self._lib.sfmba_resect_ransac(
            self._h, _capi.ptr(x), _opt_ptr(sel), _opt_ptr(use), _opt_ptr(samples), C.byref(opt), _capi.ptr(cameras),
            _capi.ptr(hyp_pose), _capi.ptr(mask), _capi.ptr(status), _capi.ptr(views), _capi.ptr(inl), _capi.ptr(best),
            _capi.ptr(sol), _capi.ptr(success), _capi.ptr(iters), _capi.ptr(rms), _opt_ptr(hyp), C.byref(n_ok), C.byref(us)))
        return RobustResection(cameras, hyp_pose, mask.view(np.bool_), status, views, inl, best, sol, success.view(np.bool_),
                               iters, rms, hyp, int(n_ok.value), float(us.value))

    def _pair_ransac(self, model, pts1, pts2, ptr, pair_use, samples, want_hyp, options, K=None):
        """What the pair-RANSAC models do alike, for one of the descriptions above: the checks, the output arrays, the
        C call -> the outputs by name (masks and ``success`` as bool), with ``n_ok``, ``kernel_us`` and the checked
        ``ptr``.  ``K``: the extra argument of a ``calibrated`` model."""
        self._flush_pending()
        batch = model.get("batch", "edge")
        pts1, pts2, ptr, use = _edge_batch(pts1, pts2, ptr, pair_use, model.get("dim", 2),
                                           model.get("names", ("pts1", "pts2", "edge_ptr")))
        if model.get("calibrated"):
            K = check_essential_args(K, options)
        E, M = ptr.shape[0] - 1, pts1.shape[0]
        opt = _capi.RansacOptions()
        self._lib.sfmba_default_ransac_options(C.byref(opt))
        what = model.get("what", "RANSAC")
        samples = _ransac_prologue(opt, options, samples, E, model["S"], f"n_{batch}s", batch, what, strict=model["strict"])
        if model.get("nan_options") and (np.isnan(opt.threshold) or np.isnan(opt.confidence)):
            raise ValueError(f"an option of the {what} is NaN")
        out = {name: np.empty((E,) + model["shape"]) for name in model["models"]}
        out.update((name, np.empty(M, dtype=np.uint8)) for name in model["masks"])
        out.update((name, np.empty(E, dtype=np.int32)) for name in model["cols"] + ("status",))
        out["success"] = np.empty(E, dtype=np.uint8)
        out.update((name, np.empty((E, int(opt.max_iters)), dtype=np.int32) if want_hyp else None) for name in model["hyps"])
        n_ok, us = C.c_int64(), C.c_double()
        order = model["models"] + model["masks"] + model["cols"] + ("success", "status") + model["hyps"]
        self._check(getattr(self._lib, model["fn"])(
            self._h, E, _capi.ptr(ptr), _capi.ptr(pts1), _capi.ptr(pts2), _opt_ptr(use), _opt_ptr(samples),
            *((_capi.ptr(K),) if model.get("calibrated") else ()), C.byref(opt), *[_opt_ptr(out[name]) for name in order],
            C.byref(n_ok), C.byref(us)))
        for name in model["masks"] + ("success",):
            out[name] = out[name].view(np.bool_)
        out.update(n_ok=n_ok.value, kernel_us=us.value, ptr=ptr)
        return out

    def fundamental_ransac(self, pts1, pts2, edge_ptr=None, pair_use=None, samples=None, want_hyp=False, **options):
        """F by RANSAC for every edge of a batch of matched pixel pairs, the reference's
        ``estimate_fundamental_matrix_ransac`` (include/sfmba.h: sfmba_fundamental_ransac).  ``pts1``, ``pts2`` (M, 2);
        ``edge_ptr`` (E + 1) the edges' runs, None = one edge; ``pair_use`` (M) boolean, None = all; ``samples``
        (E, H, 8) int32 positions among an edge's used pairs, None = drawn on the device from ``seed``.  ``options``:
        fields of ``sfmba_ransac_options`` (threshold, confidence, seed, max_iters, refit, profile); with ``samples``
        given, ``max_iters`` defaults to its H.  ``want_hyp``: also return the count of every hypothesis.  Needs no
        problem.  -> :class:`FundamentalEstimate`."""
        return FundamentalEstimate(self._pair_ransac(_FUNDAMENTAL, pts1, pts2, edge_ptr, pair_use, samples, want_hyp, options))

    def homography_ransac(self, pts1, pts2, edge_ptr=None, pair_use=None, samples=None, want_hyp=False, **options):
        """A homography ``x2 ~ H x1`` by RANSAC for every edge of a batch of matched pixel pairs (include/sfmba.h:
        sfmba_homography_ransac), the sibling of :meth:`fundamental_ransac`: the same batch arguments and the same
        ``options`` (fields of ``sfmba_ransac_options``); ``samples`` (E, H, 4) int32 positions among an edge's used
        pairs, None = drawn on the device from ``seed``; with ``samples`` given, ``max_iters`` defaults to its H.
        ``want_hyp``: also return the count of every hypothesis.  Needs no problem.  -> :class:`HomographyEstimate`."""
        return HomographyEstimate(self._pair_ransac(_HOMOGRAPHY, pts1, pts2, edge_ptr, pair_use, samples, want_hyp, options))

    def similarity_ransac(self, src, dst, set_ptr=None, pair_use=None, samples=None, want_hyp=False, **options):
        """A similarity ``dst ~ s R src + t`` by RANSAC for every set of a batch of 3-D point pairs (include/sfmba.h:
        sfmba_similarity_ransac), the fifth model of the family: ``src``, ``dst`` (M, 3); ``set_ptr`` (E + 1) the sets'
        runs, None = one set; ``pair_use`` (M) boolean, None = all; ``samples`` (E, H, 3) int32 positions among a set's used
        pairs, None = drawn on the device from ``seed``; ``options``: fields of ``sfmba_ransac_options`` -- ``threshold``
        is a distance in the units of ``dst``, so pass one --; with ``samples`` given, ``max_iters`` defaults to its H.
        ``want_hyp``: also return the count of every hypothesis.  Needs no problem.  -> :class:`SimilarityEstimate`."""
        return SimilarityEstimate(self._pair_ransac(_SIMILARITY, src, dst, set_ptr, pair_use, samples, want_hyp, options))

    def essential_ransac(self, pts1, pts2, K, edge_ptr=None, pair_use=None, samples=None, want_hyp=False, **options):
        """The essential matrix by five-point RANSAC for every edge of a batch of matched pixel pairs (include/sfmba.h:
        sfmba_essential_ransac), the calibrated sibling of :meth:`fundamental_ransac`: the same batch arguments and the
        same ``options`` (fields of ``sfmba_ransac_options``; ``refit`` must stay 0); ``K`` (3, 3) the one camera matrix of
        both images; ``samples`` (E, H, 5) int32 positions among an edge's used pairs, None = drawn on the device from
        ``seed``; with ``samples`` given, ``max_iters`` defaults to its H.  ``want_hyp``: also return the count and the
        number of real roots of every hypothesis.  Needs no problem.  -> :class:`EssentialEstimate`."""
        return EssentialEstimate(self._pair_ransac(_ESSENTIAL, pts1, pts2, edge_ptr, pair_use, samples, want_hyp, options, K=K))

    def recover_pose(self, E, pts1, pts2, K, edge_ptr=None, pair_use=None, **options):
        """R, t, the cheirality mask, the points and their ray angles for every edge of a batch, the reference's
        ``recover_pose`` (include/sfmba.h: sfmba_recover_pose).  ``E`` (n_edges, 3, 3) or (3, 3); ``K`` (3, 3); the batch
        as in :meth:`fundamental_ransac`.  ``options``: fields of ``sfmba_pose_options`` (min_depth, profile).  Needs no
        problem.  -> :class:`RelativePose`."""
        self._flush_pending()
        pts1, pts2, edge_ptr, use = _edge_batch(pts1, pts2, edge_ptr, pair_use)
        n, M = edge_ptr.shape[0] - 1, pts1.shape[0]
        E = _f64(E)
        if E.shape == (3, 3):
            E = E[None]
        E = _f64(E, (n, 3, 3), "E")
        K = _f64(K, (3, 3), "K")
        opt = _capi.PoseOptions()
        self._lib.sfmba_default_pose_options(C.byref(opt))
        _fill_options(opt, options, "pose")
        R, t = np.empty((n, 3, 3)), np.empty((n, 3))
        mask = np.empty(M, dtype=np.uint8)
        X, ang = np.empty((M, 3)), np.empty(M)
        front, status = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)
        front_all = np.empty((n, 4), dtype=np.int32)
        err = np.empty(n)
        n_ok, us = C.c_int64(), C.c_double()
        self._check(self._lib.sfmba_recover_pose(
            self._h, n, _capi.ptr(edge_ptr), _capi.ptr(pts1), _capi.ptr(pts2), _opt_ptr(use), _capi.ptr(E), _capi.ptr(K),
            C.byref(opt), _capi.ptr(R), _capi.ptr(t), _capi.ptr(mask), _capi.ptr(X), _capi.ptr(ang), _capi.ptr(front),
            _capi.ptr(front_all), _capi.ptr(err), _capi.ptr(status), C.byref(n_ok), C.byref(us)))
        return RelativePose(R, t, mask.view(np.bool_), X, ang, front, front_all, err, status, n_ok.value, us.value, edge_ptr)

    def set_descriptors(self, descs):
        """Put the descriptors of a set of images on the device: a list of (n_i, D) arrays, uint8 or anything that
        converts to float32 (include/sfmba.h: sfmba_set_descriptors).  -> the form the set takes, 1 (A: integers 0..255,
        exact) or 2 (B: general float32).  Needs no problem and leaves a set problem as it is."""
        desc, ptr = check_descriptors(descs)
        self._flush_pending()
        form = C.c_int32()
        self._check(self._lib.sfmba_set_descriptors(self._h, len(ptr) - 1, _capi.ptr(ptr), _capi.ptr(desc),
                                                    0 if desc.dtype == np.uint8 else 1, desc.shape[1], C.byref(form)))
        self.n_images, self._desc_rows = len(ptr) - 1, np.diff(ptr)
        return int(form.value)

    def match_descriptors(self, edges=None, ratio=0.5, form=0, profile=0):
        """The two nearest train descriptors of every query descriptor and Lowe's ratio test for a batch of ``edges``
        (E, 2) of (query image, train image) of the current set; None = all pairs u > v (include/sfmba.h:
        sfmba_match_descriptors).  -> :class:`DescriptorMatches`."""
        if getattr(self, "n_images", None) is None:
            raise ValueError("call set_descriptors first")
        edges = check_match_edges(edges, self.n_images)
        opt = _capi.MatchOptions()
        self._lib.sfmba_default_match_options(C.byref(opt))
        opt.ratio, opt.form, opt.profile = check_match_options(ratio, form, profile)
        self._flush_pending()
        E = edges.shape[0]
        Q = int(self._desc_rows[edges[:, 0]].sum()) if E else 0
        qptr = np.empty(E + 1, dtype=np.int64)
        idx, dist = np.empty((Q, 2), dtype=np.int32), np.empty((Q, 2))
        good = np.empty(Q, dtype=np.uint8)
        egood, status = np.empty(E, dtype=np.int32), np.empty(E, dtype=np.int32)
        n_ok, us = C.c_int64(), C.c_double()
        self._check(self._lib.sfmba_match_descriptors(
            self._h, E, _capi.ptr(edges), C.byref(opt), _capi.ptr(qptr), _capi.ptr(idx), _capi.ptr(dist), _capi.ptr(good),
            _capi.ptr(egood), _capi.ptr(status), C.byref(n_ok), C.byref(us)))
        return DescriptorMatches(edges, qptr, idx, dist, good.view(np.bool_), egood, status, n_ok.value, us.value)

    def build_tracks(self, img_ptr, edges, pair_ptr, pairs, pair_use=None, **options):
        """Feature tracks as the connected components of the used match pairs (include/sfmba.h: sfmba_build_tracks).
        ``img_ptr`` (n + 1): image i owns the global feature ids ``img_ptr[i]:img_ptr[i + 1]``; ``edges`` (E, 2) images
        (u, v); edge e owns ``pair_ptr[e]:pair_ptr[e + 1]`` of ``pairs`` (M, 2): row in u, row in v; ``pair_use`` (M) or
        None.  Options: ``min_length`` (2), ``max_length`` (0 = none), ``conflicts`` (0 drop, 1 keep), ``profile``.
        Needs no problem and no descriptors and leaves both as they are.  -> :class:`Tracks`."""
        img_ptr, edges, pair_ptr, pairs, pair_use, options = check_track_inputs(img_ptr, edges, pair_ptr, pairs, pair_use,
                                                                                **options)
        opt = _capi.TrackOptions()
        self._lib.sfmba_default_track_options(C.byref(opt))
        _fill_options(opt, options, "track")
        self._flush_pending()
        feat_track = np.empty(int(img_ptr[-1]), dtype=np.int32)
        counts, us = np.zeros(6, dtype=np.int64), C.c_double()
        self._check(self._lib.sfmba_build_tracks(
            self._h, len(img_ptr) - 1, _capi.ptr(img_ptr), len(edges), _capi.ptr(edges), _capi.ptr(pair_ptr), _capi.ptr(pairs),
            _opt_ptr(pair_use), C.byref(opt), _capi.ptr(feat_track), _capi.ptr(counts), C.byref(us)))
        track_ptr = np.empty(int(counts[1]) + 1, dtype=np.int64)
        track_feat, track_image = np.empty(int(counts[5]), dtype=np.int32), np.empty(int(counts[5]), dtype=np.int32)
        self._check(self._lib.sfmba_get_tracks(self._h, _capi.ptr(track_ptr), _capi.ptr(track_feat), _capi.ptr(track_image)))
        self._plan_dims = (len(img_ptr) - 1, int(counts[1]))               # what the masks of the plan stage are checked against
        if getattr(self, "_kp_ptr", None) is not None and not np.array_equal(self._kp_ptr, img_ptr):
            self._kp_ptr = None                                          # (the library dropped the table too)
        return Tracks(img_ptr, feat_track, track_ptr, track_feat, track_image, counts, us.value)

    def set_keypoints(self, pts_list):
        """Put the pixel positions of all features on the device, once: a list of (n_i, 2) arrays, one per image, rows as
        the tracks' feature rows (include/sfmba.h: sfmba_set_keypoints).  `assemble_problem` gathers ``points_2d`` from
        it.  Needs no tracks and no problem and leaves both as they are."""
        _, _, _, pts, ptr = check_plan_inputs(keypoints=pts_list)
        self._flush_pending()
        self._check(self._lib.sfmba_set_keypoints(self._h, len(ptr) - 1, _capi.ptr(ptr), _capi.ptr(pts)))
        self._kp_ptr = ptr

    def _plan_sizes(self):
        dims = getattr(self, "_plan_dims", None)
        if dims is None:
            raise ValueError("call build_tracks first")
        return dims

    def plan_views(self, cam_reg, trk_known, profile=0):
        """The counts a view selection needs, from the tracks of the last `build_tracks` (include/sfmba.h:
        sfmba_plan_views).  ``cam_reg`` (n_images): the image is registered; ``trk_known`` (n_tracks): the track has a 3-D
        point.  -> :class:`ViewPlan`."""
        n_images, n_tracks = self._plan_sizes()
        cam, trk, _, _, _ = check_plan_inputs(n_images, n_tracks, cam_reg, trk_known)
        opt = _capi.PlanOptions()
        self._lib.sfmba_default_plan_options(C.byref(opt))
        opt.profile = int(bool(profile))
        self._flush_pending()
        views = np.empty(n_tracks, dtype=np.int32)
        img_tracks, img_known, img_gain = (np.empty(n_images, dtype=np.int32) for _ in range(3))
        totals, us = np.zeros(3, dtype=np.int64), C.c_double()
        self._check(self._lib.sfmba_plan_views(self._h, n_images, _capi.ptr(cam), n_tracks, _capi.ptr(trk), C.byref(opt),
                                               _capi.ptr(views), _capi.ptr(img_tracks), _capi.ptr(img_known),
                                               _capi.ptr(img_gain), _capi.ptr(totals), C.byref(us)))
        return ViewPlan(cam.view(np.bool_), trk.view(np.bool_), views, img_tracks, img_known, img_gain, totals, us.value)

    def assemble_problem(self, cam_use, trk_use, min_views=2, profile=0):
        """The problem over the images of ``cam_use`` (n_images) and the tracks of ``trk_use`` (n_tracks), from the
        tracks of the last `build_tracks`: the tracks with at least ``min_views`` observations in used images, the used
        images that see one of them, renumbered index arrays and -- after `set_keypoints` -- the pixels (include/sfmba.h:
        sfmba_assemble_problem, sfmba_get_assembled).  -> :class:`SubProblem`."""
        n_images, n_tracks = self._plan_sizes()
        cam, trk, min_views, _, _ = check_plan_inputs(n_images, n_tracks, cam_use, trk_use, min_views)
        opt = _capi.PlanOptions()
        self._lib.sfmba_default_plan_options(C.byref(opt))
        opt.min_views, opt.profile = min_views, int(bool(profile))
        self._flush_pending()
        counts, us = np.zeros(3, dtype=np.int64), C.c_double()
        self._check(self._lib.sfmba_assemble_problem(self._h, n_images, _capi.ptr(cam), n_tracks, _capi.ptr(trk), C.byref(opt),
                                                     _capi.ptr(counts), C.byref(us)))
        Cn, Pn, Nn = (int(v) for v in counts)
        cam_of, pt_of = np.empty(Cn, dtype=np.int32), np.empty(Pn, dtype=np.int32)
        ci, pi, of = np.empty(Nn, dtype=np.int64), np.empty(Nn, dtype=np.int64), np.empty(Nn, dtype=np.int32)
        uv = np.empty((Nn, 2)) if getattr(self, "_kp_ptr", None) is not None else None
        self._check(self._lib.sfmba_get_assembled(self._h, _capi.ptr(cam_of), _capi.ptr(pt_of), _capi.ptr(ci), _capi.ptr(pi),
                                                  _capi.ptr(of), _opt_ptr(uv)))
        return SubProblem(cam_of, pt_of, ci, pi, of, uv, us.value)

    def residual_jacobian(self, x):
        self._flush_pending()
        x = _f64(x, (self.n_params,), "x")
        r = np.empty(2 * self.n_obs)
        Jc = np.empty((self.n_obs, 2, 6))
        Jp = np.empty((self.n_obs, 2, 3))
        self._check(self._lib.sfmba_residual_jacobian(self._h, _capi.ptr(x), _capi.ptr(r),
                                                      _capi.ptr(Jc), _capi.ptr(Jp)))
        return r, Jc, Jp

    def normal_blocks(self, x):
        self._flush_pending()
        x = _f64(x, (self.n_params,), "x")
        U = np.empty((self.n_cameras, 21))
        V = np.empty((self.n_points, 6))
        gc = np.empty((self.n_cameras, 6))
        gp = np.empty((self.n_points, 3))
        self._check(self._lib.sfmba_normal_blocks(self._h, _capi.ptr(x), _capi.ptr(U), _capi.ptr(V),
                                                  _capi.ptr(gc), _capi.ptr(gp)))
        return U, V, gc, gp

    def schur_matvec(self, x, dc, dp, v):
        self._flush_pending()
        x = _f64(x, (self.n_params,), "x")
        dc = _f64(dc).reshape(-1)
        dp = _f64(dp).reshape(-1)
        v = _f64(v).reshape(-1)
        y = np.empty(6 * self.n_cameras)
        self._check(self._lib.sfmba_schur_matvec(self._h, _capi.ptr(x), _capi.ptr(dc), _capi.ptr(dp),
                                                 _capi.ptr(v), _capi.ptr(y)))
        return y

    def step_products(self, x, sg, dc, dp_diag):
        """k_jdot and k_backsub in the selected form (include/sfmba.h: sfmba_step_products)
        -> dict(t1 (N, 2), g11, dp (P, 3), sums (10), g, si).  Both storage modes: with 32-bit storage t1 holds the
        stored float32 values exactly, g11 is the sum of the unrounded squares and sums[0] = t1.t2 uses the stored t1."""
        self._flush_pending()
        x = _f64(x, (self.n_params,), "x")
        sg = _f64(sg, (self.n_params,), "sg")
        dc, dp_diag = _f64(dc).reshape(-1), _f64(dp_diag).reshape(-1)
        if dc.shape[0] != 6 * self.n_cameras or dp_diag.shape[0] != self.n_params - 6 * self.n_cameras:
            raise ValueError("dc must hold 6 C and dp_diag 3 P entries")
        t1 = np.empty((self.n_obs, 2))
        g11 = C.c_double()
        dp = np.empty((dp_diag.shape[0] // 3, 3))
        sums, g, si = np.empty(10), np.empty(self.n_params), np.empty(self.n_params)
        self._check(self._lib.sfmba_step_products(self._h, _capi.ptr(x), _capi.ptr(sg), _capi.ptr(dc), _capi.ptr(dp_diag),
                                                  _capi.ptr(t1), C.byref(g11), _capi.ptr(dp), _capi.ptr(sums), _capi.ptr(g),
                                                  _capi.ptr(si)))
        return {"t1": t1, "g11": g11.value, "dp": dp, "sums": sums, "g": g, "si": si}

    def rhs_precond(self, x, dc, dp):
        """The rhs + preconditioner pass in the form the handle has decided (include/sfmba.h: sfmba_rhs_precond)
        -> (rhs (C, 6), sd (C, 21), minv (C, 21))."""
        self._flush_pending()
        x = _f64(x, (self.n_params,), "x")
        dc, dp = _f64(dc).reshape(-1), _f64(dp).reshape(-1)
        if dc.shape[0] != 6 * self.n_cameras or dp.shape[0] != 3 * self.n_points:
            raise ValueError("dc must hold 6 C and dp 3 P entries")
        rhs, sd, minv = np.empty((self.n_cameras, 6)), np.empty((self.n_cameras, 21)), np.empty((self.n_cameras, 21))
        self._check(self._lib.sfmba_rhs_precond(self._h, _capi.ptr(x), _capi.ptr(dc), _capi.ptr(dp), _capi.ptr(rhs),
                                                _capi.ptr(sd), _capi.ptr(minv)))
        return rhs, sd, minv

    def mixed_operands(self):
        """The fp32 operands of the mixed-precision Schur product as the last `schur_matvec` left them (include/sfmba.h:
        sfmba_get_mixed_operands) -> dict(origin (3), rt32 (C, 12) float32, rec32 (P, 8) float32, rtd (C, 12) float64).
        Raises ValueError when the problem does not run the mixed form."""
        self._flush_pending()
        origin = np.empty(3)
        rt32 = np.empty((self.n_cameras, 12), dtype=np.float32)
        rec32 = np.empty((self.n_points, 8), dtype=np.float32)
        rtd = np.empty((self.n_cameras, 12))
        self._check(self._lib.sfmba_get_mixed_operands(self._h, _capi.ptr(origin), _capi.ptr(rt32), _capi.ptr(rec32),
                                                       _capi.ptr(rtd)))
        return {"origin": origin, "rt32": rt32, "rec32": rec32, "rtd": rtd}

    ITERATION_STATE = ("scalars", "ctrl", "si", "g", "sg", "si2", "g2", "sg2", "Dc", "Minv", "Vinv", "e", "pcg_x", "pcg_r",
                       "p", "x_new")

    def iteration_state(self, skip=()):
        """What the last outer iteration of the last `solve` left on the handle (include/sfmba.h:
        sfmba_get_iteration_state) -> dict of ITERATION_STATE without the names of ``skip``: scalars (32), ctrl (dict:
        rz, rz0, tol2, rz_prev, alpha_prev, iters, max_iters, done), si, g, sg, si2, g2, sg2, p, x_new (n), Dc (C, 6),
        Minv (C, 21), Vinv (P, 6), e (P, 3), pcg_x, pcg_r (C, 6).  An output the solve's form does not keep has to be in
        ``skip``: asking for it raises ValueError.  Copies only."""
        unknown = set(skip) - set(self.ITERATION_STATE)
        if unknown:
            raise ValueError(f"unknown outputs {sorted(unknown)}")
        self._flush_pending()
        nc, npt, n = self.n_cameras, self.n_points, self.n_params
        shapes = {"scalars": (32,), "ctrl": (8,), "Dc": (nc, 6), "Minv": (nc, 21), "Vinv": (npt, 6), "e": (npt, 3),
                  "pcg_x": (nc, 6), "pcg_r": (nc, 6)}
        out = {name: np.empty(shapes.get(name, (n,))) for name in self.ITERATION_STATE if name not in skip}
        self._check(self._lib.sfmba_get_iteration_state(self._h, *[_opt_ptr(out.get(name)) for name in self.ITERATION_STATE]))
        if "ctrl" in out:
            c = out["ctrl"]
            out["ctrl"] = {"rz": float(c[0]), "rz0": float(c[1]), "tol2": float(c[2]), "rz_prev": float(c[3]),
                           "alpha_prev": float(c[4]), "iters": int(c[5]), "max_iters": int(c[6]), "done": int(c[7])}
        return out

    def dense_schur(self, x, dc, dp, rhs):
        """(S, y): the formed reduced camera matrix and the solution of S y = rhs by the in-LDS PCG run to the end."""
        self._flush_pending()
        x = _f64(x, (self.n_params,), "x")
        dc, dp, rhs = _f64(dc).reshape(-1), _f64(dp).reshape(-1), _f64(rhs).reshape(-1)
        n = 6 * self.n_cameras
        S = np.empty((n, n))
        y = np.empty(n)
        self._check(self._lib.sfmba_dense_schur(self._h, _capi.ptr(x), _capi.ptr(dc), _capi.ptr(dp), _capi.ptr(rhs),
                                                _capi.ptr(S), _capi.ptr(y)))
        return S, y

    def time_kernel(self, x, which: int, reps: int) -> float:
        self._flush_pending()
        x = _f64(x, (self.n_params,), "x")
        us = C.c_double()
        self._check(self._lib.sfmba_time_kernel(self._h, _capi.ptr(x), int(which), int(reps),
                                                C.byref(us)))
        return us.value

    def default_options(self) -> _capi.Options:
        o = _capi.Options()
        self._lib.sfmba_default_options(C.byref(o))
        return o

    def solve(self, x0, options: _capi.Options | None = None, want_fun=True, want_grad=True):
        """-> (x, result struct, fun, grad).  fun / grad not wanted stay on the device: `fetch_fun_grad` gets them
        until the next operation on this handle."""
        self._flush_pending()
        x_start = _f64(x0, (self.n_params,), "x0")
        x = np.empty_like(x_start)               # start and result in separate arrays: no copy of x0 on the way in
        opt = options if options is not None else self.default_options()
        res = _capi.Result()
        self._check(self._lib.sfmba_solve_from(self._h, _capi.ptr(x_start), _capi.ptr(x), C.byref(opt), C.byref(res)))
        fun, grad = self.fetch_fun_grad(want_fun, want_grad)
        return x, res, fun, grad
