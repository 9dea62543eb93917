"""Helpers either side of the hot path: reprojection-error reporting in the pipeline's
``[R | t]`` convention, calibration / problem files.  Numeric work still goes through the HIP path."""
from __future__ import annotations

import numpy as np

from . import _capi, api
from .backend import check_descriptors, check_essential_args, check_match_edges, check_match_options, check_track_inputs


def reproj_error(point3ds, point2ds, K, R, tvec, device=0):
    """``(K (R X + t))`` projected minus ``point2ds`` -> (N,2), as
    /root/reference/cv2_lite/solve_pnp.py:9-15.  Evaluated by the BA residual kernel: ``R X + t`` equals
    the kernel's ``R (X - T)`` with the camera centre ``T = -R^T t``."""
    point3ds = np.ascontiguousarray(point3ds, dtype=np.float64)
    point2ds = np.ascontiguousarray(point2ds, dtype=np.float64)
    R = np.asarray(R, dtype=np.float64)
    tvec = np.asarray(tvec, dtype=np.float64).reshape(3)
    n = len(point3ds)
    if point3ds.shape != (n, 3) or point2ds.shape != (n, 2) or np.shape(K) != (3, 3):
        raise ValueError("expected point3ds (N,3), point2ds (N,2), K (3,3)")   # check_inputs.py:7-48
    cam = np.hstack([api._rotvec_from_matrix(R), -R.T @ tvec])
    x = np.concatenate([cam, point3ds.ravel()])
    r = api.compute_residuals(x, 1, n, np.zeros(n, dtype=np.int64), np.arange(n, dtype=np.int64), point2ds, K,
                              device=device)
    return r.reshape(n, 2)


def calc_reproj_error(points3d, points2d, K, R, tvec, device=0):
    """Mean L2 reprojection error, /root/reference/sfm_lite/sfm.py:38-41."""
    return float(np.linalg.norm(reproj_error(points3d, points2d, K, R, tvec, device=device), axis=1).mean())


def _backend_with_problem(args, device, backend):
    n_cameras, n_points, camera_indices, point_indices, points_2d, K = api._split_args(tuple(args))
    be = backend if backend is not None else api.get_backend(device)
    be.set_precision(64)
    be.set_fixed_cameras(())
    be.set_problem(n_cameras, n_points, camera_indices, point_indices, points_2d, K)
    return be


def reprojection_stats(x, args, max_error_px=np.inf, min_depth=-np.inf, min_angle_deg=0.0, min_views=0,
                       want=("obs", "points", "cameras"), device=0, backend=None):
    """`Backend.reprojection_stats` in one call on the reference's ``args`` tuple (sfm.py:268): per-observation
    reprojection error, depth and keep mask, per-point track statistics, per-camera error statistics and a summary at
    ``x``, evaluated by one sweep on the device.  ``backend``: a :class:`Backend` to run on instead of the calling
    thread's own (``device`` is then ignored)."""
    be = _backend_with_problem(args, device, backend)
    return be.reprojection_stats(x, max_error_px=max_error_px, min_depth=min_depth, min_angle_deg=min_angle_deg,
                                 min_views=min_views, want=want)


def covariance(x, n_cameras, n_points, camera_indices, point_indices, points_2d, K, fixed_camera_indices=(), device=0,
               backend=None, **kw):
    """Camera and point covariance blocks of a bundle-adjustment solution ``x`` on the arguments of the reference's
    ``least_squares`` call (`Backend.covariance`; include/sfmba.h: sfmba_covariance).  ``fixed_camera_indices``: cameras the
    problem holds still, as ``create_sparsity_matrix`` takes them; ``kw``: ``hold`` (indices 6 c + k or (camera, component)
    pairs), ``kind``, ``gauge``, ``sigma2``, ``want_full``, ``want_points``, ``rank_tol``, ``point_tol``, ``profile``.
    ``backend``: a :class:`Backend` to run on instead of the calling thread's own (``device`` is then ignored)."""
    be = backend if backend is not None else api.get_backend(device)
    be.set_precision(64)
    be.set_fixed_cameras(fixed_camera_indices)
    be.set_problem(n_cameras, n_points, camera_indices, point_indices, points_2d, K)
    return be.covariance(x, **kw)


def total_mean_reproj_error(x, args, device=0, backend=None):
    """Mean L2 reprojection error over all observations at ``x``: the figure the reference accumulates after every fused
    edge with one ``calc_reproj_error`` call per observation (sfm.py:234-241), here from one sweep.

    Two things the reference does are documented, not imitated.  It divides the sum by the LAST LOOP INDEX ``n = N - 1``
    (``enumerate`` starts at 0) and not by the number of observations; this function divides by ``N``, so the
    reference's printed value is ``N / (N - 1)`` times larger.  And it reads a pose ``H`` as ``[R | t]`` with
    ``x_cam = R X + t``, while the bundle-adjustment model -- and ``x`` here -- holds the camera
    CENTRE, ``x_cam = R (X - T)``; pack poses with ``pack_cameras_points(..., pose_convention=...)`` accordingly."""
    st = reprojection_stats(x, args, want=(), device=device, backend=backend)
    return st.sum_err / max(st.n_obs, 1)


def prune_problem(x, args, obs_keep, pt_keep):
    """Remove dropped observations and dropped points from a problem -> ``(x2, args2, obs_index, point_index)``.

    ``obs_keep`` (N) and ``pt_keep`` (P) are boolean masks, e.g. those of :func:`reprojection_stats`.  An observation
    survives when it is kept AND its point is kept; a point survives when it is kept (an observation of a dropped point
    goes with it).  Points are renumbered densely in their old order, observations keep their order, ALL cameras stay
    (their indices remain valid; a camera left without observations is legal input to the solver).  ``obs_index`` and
    ``point_index`` are the positions of the surviving rows in the original arrays: ``args2``'s pixels are
    ``points_2d[obs_index]``, the points of ``x2`` are those of ``x`` at ``point_index``.  Pure numpy."""
    n_cameras, n_points, camera_indices, point_indices, points_2d, K = api._split_args(tuple(args))
    n_cameras, n_points = int(n_cameras), int(n_points)
    ci = np.asarray(camera_indices).ravel()
    pi = np.asarray(point_indices).ravel()
    p2 = np.asarray(points_2d)
    x = np.asarray(x, dtype=np.float64).ravel()
    obs_keep = np.asarray(obs_keep).ravel()
    pt_keep = np.asarray(pt_keep).ravel()
    if obs_keep.shape[0] != ci.shape[0] or pi.shape[0] != ci.shape[0] or p2.shape[0] != ci.shape[0]:
        raise ValueError(f"obs_keep has {obs_keep.shape[0]} entries, the problem {ci.shape[0]} observations")
    if pt_keep.shape[0] != n_points:
        raise ValueError(f"pt_keep has {pt_keep.shape[0]} entries, the problem {n_points} points")
    if x.shape[0] != 6 * n_cameras + 3 * n_points:
        raise ValueError(f"x has {x.shape[0]} entries, expected 6*n_cameras + 3*n_points = {6 * n_cameras + 3 * n_points}")
    pt_keep = pt_keep.astype(bool)
    obs_index = np.flatnonzero(obs_keep.astype(bool) & pt_keep[pi])
    point_index = np.flatnonzero(pt_keep)
    new_id = np.full(n_points, -1, dtype=np.int64)
    new_id[point_index] = np.arange(point_index.shape[0], dtype=np.int64)
    pts = x[6 * n_cameras:].reshape(n_points, 3)
    x2 = np.concatenate([x[:6 * n_cameras], pts[point_index].ravel()])
    args2 = (n_cameras, int(point_index.shape[0]), ci[obs_index], new_id[pi[obs_index]], p2[obs_index], K)
    return x2, args2, obs_index, point_index


def triangulate_tracks(x, args, select=None, obs_use=None, device=0, backend=None, **options):
    """`Backend.triangulate` in one call on the reference's ``args`` tuple (sfm.py:268): every selected point from all its
    used observations and the cameras of ``x`` -- n-view DLT, Gauss-Newton on the reprojection error, a verdict per point
    -- by one kernel on the device.  ``options``: the fields of ``sfmba_triangulate_options``.
    -> :class:`sfmba.Triangulation`."""
    be = _backend_with_problem(args, device, backend)
    return be.triangulate(x, select=select, obs_use=obs_use, **options)


def triangulate_tracks_ransac(x, args, select=None, obs_use=None, want_hyp=False, device=0, backend=None, **options):
    """`Backend.triangulate_ransac` in one call on the reference's ``args`` tuple (sfm.py:268): every selected point by a
    RANSAC over pairs of its used observations, then :func:`triangulate_tracks` over the inliers of the best pair --
    one wrong observation costs a track that observation, not the point.  ``options``: the fields of
    ``sfmba_tri_ransac_options``.  -> :class:`RobustTriangulation`."""
    be = _backend_with_problem(args, device, backend)
    return be.triangulate_ransac(x, select=select, obs_use=obs_use, want_hyp=want_hyp, **options)


def resect_cameras(x, args, select=None, obs_use=None, device=0, backend=None, **options):
    """`Backend.resect` in one call on the reference's ``args`` tuple (sfm.py:268): every selected camera from all its used
    observations and the points of ``x`` -- n-point DLT, Gauss-Newton on the reprojection error over the pose, a verdict
    per camera -- by one kernel on the device.  ``options``: the fields of ``sfmba_resect_options``.
    -> :class:`sfmba.Resection`."""
    be = _backend_with_problem(args, device, backend)
    return be.resect(x, select=select, obs_use=obs_use, **options)


def solve_pnp(point3ds, point2ds, K, dist=None, device=0, backend=None, **options):
    """``cv2.solvePnP(point3ds, point2ds, K, dist)`` as the reference calls it (sfm.py:207-208): ``(N, 3)`` points and
    ``(N, 2)`` pixels -> ``(success, rvec (3, 1), tvec (3, 1))`` in OpenCV's ``x_cam = R X + t`` convention.  A one-camera
    problem through :func:`resect_cameras`: ``success`` is ``status == OK``, and a pose that is not OK comes back as NaN.
    The device model has no lens distortion: a non-zero ``dist`` raises ValueError.  ``options``: the fields of
    ``sfmba_resect_options`` (``max_iter=0`` gives the linear stage alone)."""
    if dist is not None and np.any(np.asarray(dist, dtype=np.float64) != 0.0):
        raise ValueError("solve_pnp supports no lens distortion: dist must be None or all zeros")
    point3ds = np.ascontiguousarray(point3ds, dtype=np.float64)
    point2ds = np.ascontiguousarray(point2ds, dtype=np.float64)
    n = len(point3ds)
    if point3ds.shape != (n, 3) or point2ds.shape != (n, 2) or np.shape(K) != (3, 3):
        raise ValueError("expected point3ds (N,3), point2ds (N,2), K (3,3)")
    x = np.concatenate([np.zeros(6), point3ds.ravel()])
    res = resect_cameras(x, (1, n, np.zeros(n, dtype=np.int64), np.arange(n, dtype=np.int64), point2ds, K),
                         device=device, backend=backend, **options)
    if not res.ok[0]:
        return False, np.full((3, 1), np.nan), np.full((3, 1), np.nan)
    w, T = res.cameras[0, :3], res.cameras[0, 3:]
    R = api._matrix_from_rotvec(w)
    return True, w.reshape(3, 1).copy(), (-R @ T).reshape(3, 1)


def resect_cameras_ransac(x, args, select=None, obs_use=None, samples=None, want_hyp=False, device=0, backend=None, **options):
    """`Backend.resect_ransac` in one call on the reference's ``args`` tuple (sfm.py:268): every selected camera by P3P
    inside RANSAC over its used observations, then the pose refinement of :func:`resect_cameras` over the inliers -- the
    registration step that survives wrong 2-D--3-D correspondences.  ``options``: the fields of
    ``sfmba_pnp_ransac_options``.  -> :class:`sfmba.RobustResection`."""
    be = _backend_with_problem(args, device, backend)
    return be.resect_ransac(x, select=select, obs_use=obs_use, samples=samples, want_hyp=want_hyp, **options)


def solve_pnp_ransac(objectPoints, imagePoints, K, dist=None, iterationsCount=100, reprojectionError=8.0, confidence=0.99,
                     seed=0, device=0, backend=None, **options):
    """``cv2.solvePnPRansac(objectPoints, imagePoints, K, dist, iterationsCount=, reprojectionError=, confidence=)``:
    ``(N, 3)`` points and ``(N, 2)`` pixels -> ``(retval, rvec (3, 1), tvec (3, 1), inliers (k, 1) int32)`` in OpenCV's
    ``x_cam = R X + t`` convention, ``inliers`` the positions of the inlier correspondences.  A one-camera problem through
    :func:`resect_cameras_ransac`: ``retval`` is ``status == OK``; a failure gives False, NaN poses and an empty
    ``inliers``.  ``confidence`` only feeds ``cam_success`` (there is no adaptive exit: all ``iterationsCount`` hypotheses
    run).  The device model has no lens distortion: a non-zero ``dist`` raises ValueError.  ``options``: further fields of
    ``sfmba_pnp_ransac_options`` (min_views, refine, min_depth, max_iter, xtol, max_rms_px)."""
    if dist is not None and np.any(np.asarray(dist, dtype=np.float64) != 0.0):
        raise ValueError("solve_pnp_ransac supports no lens distortion: dist must be None or all zeros")
    objectPoints = np.ascontiguousarray(objectPoints, dtype=np.float64)
    imagePoints = np.ascontiguousarray(imagePoints, dtype=np.float64)
    n = len(objectPoints)
    if objectPoints.shape != (n, 3) or imagePoints.shape != (n, 2) or np.shape(K) != (3, 3):
        raise ValueError("expected objectPoints (N,3), imagePoints (N,2), K (3,3)")
    if int(iterationsCount) < 1:
        raise ValueError("iterationsCount must be at least 1")
    x = np.concatenate([np.zeros(6), objectPoints.ravel()])
    res = resect_cameras_ransac(x, (1, n, np.zeros(n, dtype=np.int64), np.arange(n, dtype=np.int64), imagePoints, K),
                                device=device, backend=backend, max_iters=int(iterationsCount),
                                threshold=float(reprojectionError), confidence=float(confidence), seed=seed, **options)
    if not res.ok[0]:
        return False, np.full((3, 1), np.nan), np.full((3, 1), np.nan), np.zeros((0, 1), dtype=np.int32)
    w, T = res.cameras[0, :3], res.cameras[0, 3:]
    R = api._matrix_from_rotvec(w)
    return True, w.reshape(3, 1).copy(), (-R @ T).reshape(3, 1), np.flatnonzero(res.inlier_mask).astype(np.int32).reshape(-1, 1)


def _cameras_from_projection(M, K):
    """``[R | t] = K^-1 M`` -> (rotation vector, centre ``T = -R^T t``), the six camera parameters of the
    bundle-adjustment model.  Raises ValueError when ``R`` is not a rotation to within 1e-6."""
    M = np.asarray(M, dtype=np.float64)
    if M.shape != (3, 4):
        raise ValueError(f"a projection matrix has shape (3, 4), got {M.shape}")
    Rt = np.linalg.solve(np.asarray(K, dtype=np.float64), M)
    R, t = Rt[:, :3], Rt[:, 3]
    if not (np.all(np.isfinite(R)) and np.abs(R.T @ R - np.eye(3)).max() <= 1e-6 and abs(np.linalg.det(R) - 1.0) <= 1e-6):
        raise ValueError("K^-1 M[:, :3] is not a rotation to within 1e-6: M is not K [R | t] for this K")
    return np.concatenate([api._rotvec_from_matrix(R), -R.T @ t])


def triangulate_points(M1, M2, pts1, pts2, K, device=0, backend=None):
    """``cv2.triangulatePoints(M1, M2, pts1, pts2)`` as the reference calls it (sfm.py:140, 218): ``(3, 4)`` projection
    matrices ``K [R | t]`` and ``(2, N)`` pixels -> ``(4, N)`` homogeneous points with last row 1.  The linear stage of
    :func:`triangulate_tracks` alone (no refinement, no angle, depth or error test) on a two-camera problem built from
    ``[R | t] = K^-1 M``; a point at infinity comes back as a NaN column.  ``K`` is needed because the device model holds
    rotations, not general 3x4 matrices."""
    if np.shape(K) != (3, 3):
        raise ValueError("K must be (3, 3)")
    cams = np.concatenate([_cameras_from_projection(M1, K), _cameras_from_projection(M2, K)])
    pts1, pts2 = np.asarray(pts1, dtype=np.float64), np.asarray(pts2, dtype=np.float64)
    if pts1.ndim != 2 or pts1.shape[0] != 2 or pts1.shape != pts2.shape:
        raise ValueError(f"pts1 and pts2 must both be (2, N), got {pts1.shape} and {pts2.shape}")
    n = pts1.shape[1]
    out = np.ones((4, n))
    if n == 0:
        return out
    uv = np.stack([pts1.T, pts2.T], axis=1).reshape(2 * n, 2)            # point-major: (view 1, view 2) per point
    ci = np.tile(np.array([0, 1], dtype=np.int64), n)
    pi = np.repeat(np.arange(n, dtype=np.int64), 2)
    be = _backend_with_problem((2, n, ci, pi, uv, K), device, backend)
    tri = be.triangulate(np.concatenate([cams, np.zeros(3 * n)]), max_iter=0, min_views=2, min_angle_deg=-np.inf,
                         min_depth=-np.inf, max_error_px=np.inf)
    out[:3] = np.where(tri.ok[None, :], tri.points.T, np.nan)
    return out


def refine_reconstruction(x0, args, rounds=2, max_error_px=4.0, min_depth=0.0, min_angle_deg=2.0, min_views=2,
                          device=0, backend=None, retriangulate=False, **least_squares_kwargs):
    """The trim loop around bundle adjustment: solve, measure, drop, solve again.

    Every round solves the current problem with :func:`sfmba.least_squares` (``least_squares_kwargs`` are passed on;
    ``x_scale='jac'`` and ``method='trf'`` are the defaults), takes :func:`reprojection_stats` at the result with the
    four thresholds and prunes what fails them (:func:`prune_problem`).  It stops after ``rounds`` solves, or as soon as
    a round drops nothing.  -> ``(result, (x, args), (obs_index, point_index), summaries)``: the last solve's result; the
    surviving problem with the parameters at the last solve's ``x``; the surviving rows' positions in the ORIGINAL
    arrays, composed over all rounds; per round a dict with ``n_obs``, ``n_points`` (solved), ``n_obs_kept``,
    ``n_points_kept``, ``mean_error_px``, ``rms_error_px``, ``max_error_px`` (over the kept set) and ``rmse`` (the
    solve's, over everything it was given).

    ``retriangulate=True`` gives the points a round would drop a second chance before it drops them: every such point
    with at least ``max(2, min_views)`` observations is triangulated anew (:meth:`Backend.triangulate`, same four
    thresholds) from its observations that pass their own test -- from all its observations when fewer than
    ``min_views`` pass, the case of a point that is itself misplaced while its pixels are fine.  A point that comes back
    ``OK`` takes its new coordinates, the statistics are taken again at the updated ``x``, and the pruning follows those:
    the point stays, observations of it that still fail are dropped.  Each summary then carries
    ``n_points_retriangulated``, the points rescued in that round."""
    if rounds < 1:
        raise ValueError("rounds must be at least 1")
    kw = dict(x_scale="jac", method="trf")
    kw.update(least_squares_kwargs)
    be = backend if backend is not None else api.get_backend(device)
    x = np.asarray(x0, dtype=np.float64).ravel()
    args = api._split_args(tuple(args))
    obs_index = np.arange(len(np.asarray(args[2]).ravel()), dtype=np.int64)
    point_index = np.arange(int(args[1]), dtype=np.int64)
    summaries = []
    result = None
    for _ in range(int(rounds)):
        result = api.least_squares(api.compute_residuals, x, args=args, backend=be, **kw)
        # (the handle holds exactly this problem: statistics straight on it, in the solve's storage precision)
        st = be.reprojection_stats(result.x, max_error_px=max_error_px, min_depth=min_depth, min_angle_deg=min_angle_deg,
                                   min_views=min_views, want=("obs", "points"))
        x = result.x
        n_retriangulated = 0
        if retriangulate and st.n_points_kept < int(args[1]):
            pidx = np.asarray(args[3]).ravel()
            own = (st.obs_err <= max_error_px) & np.isfinite(st.obs_err) & (st.obs_depth > min_depth)
            need = max(2, int(min_views))
            cand = ~st.pt_keep & (np.bincount(pidx, minlength=int(args[1])) >= need)
            if cand.any():
                tri = be.triangulate(x, select=cand, obs_use=own | (st.pt_views < need)[pidx], min_views=min_views,
                                     min_angle_deg=min_angle_deg, min_depth=min_depth, max_error_px=max_error_px)
                n_retriangulated = tri.n_ok
                if n_retriangulated:
                    x = np.concatenate([x[:6 * int(args[0])], tri.points.ravel()])
                    st = be.reprojection_stats(x, max_error_px=max_error_px, min_depth=min_depth,
                                               min_angle_deg=min_angle_deg, min_views=min_views, want=("obs", "points"))
        summaries.append(dict(n_obs=st.n_obs, n_points=int(args[1]), n_obs_kept=st.n_obs_kept,
                              n_points_kept=st.n_points_kept, mean_error_px=st.mean_error_px,
                              rms_error_px=st.rms_error_px, max_error_px=st.max_err, rmse=float(result.rmse)))
        if retriangulate:
            summaries[-1]["n_points_retriangulated"] = int(n_retriangulated)
        if st.n_obs_kept == st.n_obs and st.n_points_kept == int(args[1]):
            break
        x, args, oi, pi = prune_problem(x, args, st.obs_keep, st.pt_keep)
        obs_index, point_index = obs_index[oi], point_index[pi]
    return result, (x, args), (obs_index, point_index), summaries


FM_RANSAC = 8        # cv2.FM_RANSAC, the one method of the reference's teaching restatement


def find_fundamental_mat(pts1, pts2, method=FM_RANSAC, ransacReprojThreshold=3.0, confidence=0.99, maxIters=1000, seed=0,
                         device=0, backend=None):
    """The two-line swap for ``cv2.findFundamentalMat(pts1, pts2, cv2.FM_RANSAC, thr, conf)`` (sfm.py:101) ->
    ``(F (3, 3), mask (N, 1) uint8)`` as cv2 returns them; ``F`` is ``None`` when the pairs give no F.  One call of
    :meth:`Backend.fundamental_ransac` with ``refit=1``: the F returned is the refit over all inliers of the best
    hypothesis.  The score is the REFERENCE's (one-sided distance in image 2, strictly below the threshold), not cv2's
    symmetric one; the samples are drawn on the device from ``seed``."""
    if method != FM_RANSAC:
        raise ValueError("only method=FM_RANSAC is implemented")
    pts1, pts2 = np.asarray(pts1, dtype=np.float64), np.asarray(pts2, dtype=np.float64)
    if pts1.ndim != 2 or pts1.shape[1] != 2 or pts1.shape != pts2.shape:
        raise ValueError(f"pts1 and pts2 must both be (N, 2), got {pts1.shape} and {pts2.shape}")
    be = backend if backend is not None else api.get_backend(device)
    est = be.fundamental_ransac(pts1, pts2, threshold=ransacReprojThreshold, confidence=confidence, max_iters=maxIters,
                                seed=seed, refit=1)
    mask = est.inlier_mask.astype(np.uint8).reshape(-1, 1)
    return (est.F_refit[0].copy() if est.status[0] == est.OK else None), mask


def recover_pose(E, pts1, pts2, K, device=0, backend=None):
    """The two-line swap for ``cv2.recoverPose(E, pts1, pts2, K)`` (sfm.py:131) -> ``(n_front, R (3, 3), t (3, 1), mask
    (N, 1) uint8 of 0 / 255)``: one call of :meth:`Backend.recover_pose`."""
    pts1, pts2 = np.asarray(pts1, dtype=np.float64), np.asarray(pts2, dtype=np.float64)
    if pts1.ndim != 2 or pts1.shape[1] != 2 or pts1.shape != pts2.shape:
        raise ValueError(f"pts1 and pts2 must both be (N, 2), got {pts1.shape} and {pts2.shape}")
    if np.shape(E) != (3, 3) or np.shape(K) != (3, 3):
        raise ValueError("E and K must be (3, 3)")
    be = backend if backend is not None else api.get_backend(device)
    pose = be.recover_pose(E, pts1, pts2, K)
    return int(pose.front[0]), pose.R[0].copy(), pose.t[0].reshape(3, 1).copy(), pose.front_mask.astype(np.uint8).reshape(-1, 1) * 255


RANSAC = 8           # cv2.RANSAC, the one method of find_homography


def find_homography(srcPoints, dstPoints, method=RANSAC, ransacReprojThreshold=3.0, maxIters=2000, confidence=0.995, seed=0,
                    device=0, backend=None):
    """The swap for ``cv2.findHomography(srcPoints, dstPoints, cv2.RANSAC, thr)`` -> ``(H (3, 3) scaled to H[2, 2] = 1,
    mask (N, 1) uint8)``; ``H`` is ``None`` when the pairs give no homography.  One call of
    :meth:`Backend.homography_ransac` with ``refit=1``: ``H`` is ``H_refit``, the estimate over all inliers of the best
    hypothesis, and ``mask`` is ``refit_mask``, so the mask belongs to the matrix returned.  ``H`` stays of unit norm when
    ``|H[2, 2]|`` is below 1e-12.  The defaults are cv2's; ``confidence`` only decides ``success`` of the batch call, every
    one of the ``maxIters`` hypotheses is scored.  Not done: the Levenberg-Marquardt refinement cv2 runs after its RANSAC."""
    if method != RANSAC:
        raise ValueError("only method=RANSAC is implemented")
    src, dst = np.asarray(srcPoints, dtype=np.float64), np.asarray(dstPoints, dtype=np.float64)
    if src.ndim == 3 and src.shape[1] == 1:                       # cv2's (N, 1, 2)
        src = src[:, 0]
    if dst.ndim == 3 and dst.shape[1] == 1:
        dst = dst[:, 0]
    if src.ndim != 2 or src.shape[1] != 2 or src.shape != dst.shape:
        raise ValueError(f"srcPoints and dstPoints must both be (N, 2), got {src.shape} and {dst.shape}")
    be = backend if backend is not None else api.get_backend(device)
    est = be.homography_ransac(src, dst, threshold=ransacReprojThreshold, confidence=confidence, max_iters=maxIters, seed=seed,
                               refit=1)
    mask = est.refit_mask.astype(np.uint8).reshape(-1, 1)
    if est.status[0] != est.OK:
        return None, mask
    H = est.H_refit[0].copy()
    if abs(H[2, 2]) >= 1e-12:
        H = H / H[2, 2]
        H[2, 2] = 1.0
    return H, mask


def find_essential_mat(points1, points2, cameraMatrix, method=RANSAC, prob=0.999, threshold=1.0, maxIters=1000, seed=0, device=0,
                       backend=None):
    """The swap for ``cv2.findEssentialMat(points1, points2, cameraMatrix, cv2.RANSAC, prob, threshold)`` -> ``(E (3, 3),
    mask (N, 1) uint8)``; ``E`` is ``None`` when the pairs give no essential matrix.  One call of
    :meth:`Backend.essential_ransac`: ``E`` is the best five-point candidate itself (unit norm; there is no refit), ``mask``
    its inliers.  The score is the F call's one-sided distance in image 2 in pixels, not cv2's Sampson distance; ``prob`` only
    decides ``success`` of the batch call, every one of the ``maxIters`` hypotheses is scored."""
    if method != RANSAC:
        raise ValueError("only method=RANSAC is implemented")
    p1, p2 = np.asarray(points1, dtype=np.float64), np.asarray(points2, dtype=np.float64)
    if p1.ndim == 3 and p1.shape[1] == 1:                         # cv2's (N, 1, 2)
        p1 = p1[:, 0]
    if p2.ndim == 3 and p2.shape[1] == 1:
        p2 = p2[:, 0]
    if p1.ndim != 2 or p1.shape[1] != 2 or p1.shape != p2.shape:
        raise ValueError(f"points1 and points2 must both be (N, 2), got {p1.shape} and {p2.shape}")
    Km = check_essential_args(cameraMatrix, {})
    be = backend if backend is not None else api.get_backend(device)
    est = be.essential_ransac(p1, p2, Km, threshold=threshold, confidence=prob, max_iters=maxIters, seed=seed)
    mask = est.inlier_mask.astype(np.uint8).reshape(-1, 1)
    return (est.E[0].copy() if est.status[0] == est.OK else None), mask


def select_initial_pair(edges, K, min_angle=3, max_angle=60, device=0, backend=None, max_homography_ratio=None,
                        two_view="fundamental", **ransac_options):
    """The first-pair choice of ``SFM._initial_register`` (sfm.py:120-180) for a list ``edges`` of ``(pts1, pts2)``: one
    :meth:`Backend.fundamental_ransac` call (``refit=1``) and one :meth:`Backend.recover_pose` call (``E = K^T F K``, over
    each edge's inliers) for the whole list, then on the host the median of ``angle_deg`` over each edge's pairs in front.
    -> ``(index, R, t, X, mask)``: the edge with the smallest median strictly inside ``(min_angle, max_angle)`` degrees
    (the reference's ``3 < mid_angle < 60``) among the edges whose F and pose both came back ``OK``, its pose,
    its points ``X`` (N, 3; NaN where not in front) and its front mask (N) -- or ``(None, None, None, None, None)``.

    The reference's own angle code sums over the wrong axis (sfm.py:153-154 take ``axis=0`` on (N, 3) arrays, which mixes
    the pairs); this is the per-pair angle between the two rays that it intends.  One more deviation: an edge whose pose
    is a ``TIE`` (two candidates see equally many pairs in front) is passed over, where the reference takes whichever
    candidate ``max`` meets first: an ambiguous pose is no start for a reconstruction.

    ``max_homography_ratio``: None (the default) makes exactly the calls above.  With a number, one
    :meth:`Backend.homography_ransac` call over the same batch (the same threshold, ``max_iters`` and seed, ``refit=1``) is
    added, and an edge whose support ratio ``H.refit_inliers / F.inliers`` exceeds it, or whose F count is 0, is passed
    over: a planar scene or a pure rotation supports a two-parameter family of F, the F fitted there is whatever the
    noise makes it, and its median angle is a small number that often lands inside the window.  Prototyped in numpy on the
    CPU (300 pairs, 0.3 px noise, 25 % outliers, threshold 1 px, 100 hypotheses, one generator at one seed), the ratio was
    0.92-0.98 on four planar edges, 0.91-1.00 on four pure-rotation edges and 0.02-0.04 on four general edges (the 4-6
    pairs a four-point H always fits); COLMAP's customary value is 0.8.

    ``two_view``: ``"fundamental"`` (the default) makes exactly the calls above.  With ``"essential"`` one
    :meth:`Backend.essential_ransac` call takes the place of the F call (``refit`` is not passed on) and its ``E`` goes to
    :meth:`Backend.recover_pose` as it is; the homography gate then compares against the E count."""
    if two_view not in ("fundamental", "essential"):
        raise ValueError(f"two_view must be 'fundamental' or 'essential', got {two_view!r}")
    if max_homography_ratio is not None and not float(max_homography_ratio) >= 0.0:
        raise ValueError(f"max_homography_ratio must be None or a non-negative number, got {max_homography_ratio!r}")
    if not len(edges):
        raise ValueError("edges is empty")
    K = np.asarray(K, dtype=np.float64)
    if K.shape != (3, 3):
        raise ValueError("K must be (3, 3)")
    p1 = [np.asarray(e[0], dtype=np.float64) for e in edges]
    p2 = [np.asarray(e[1], dtype=np.float64) for e in edges]
    for a, b in zip(p1, p2):
        if a.ndim != 2 or a.shape[1] != 2 or a.shape != b.shape:
            raise ValueError(f"every edge must be a pair of (N, 2) arrays, got {a.shape} and {b.shape}")
    ptr = np.concatenate([[0], np.cumsum([len(a) for a in p1])]).astype(np.int64)
    pts1, pts2 = np.concatenate(p1), np.concatenate(p2)
    be = backend if backend is not None else api.get_backend(device)
    if two_view == "essential":
        check_essential_args(K, ransac_options)
        est = be.essential_ransac(pts1, pts2, K, edge_ptr=ptr, **ransac_options)
        E = est.E
    else:
        ransac_options.setdefault("refit", 1)
        est = be.fundamental_ransac(pts1, pts2, edge_ptr=ptr, **ransac_options)
        E = np.einsum("ji,ejk,kl->eil", K, est.F_refit, K)
    pose = be.recover_pose(E, pts1, pts2, K, edge_ptr=ptr, pair_use=est.inlier_mask)
    planar = np.zeros(len(edges), dtype=bool)
    if max_homography_ratio is not None:
        hom = be.homography_ransac(pts1, pts2, edge_ptr=ptr, **{**ransac_options, "refit": 1})
        planar = (est.inliers <= 0) | (hom.refit_inliers > float(max_homography_ratio) * est.inliers)
    best, best_median = None, np.inf
    for e in range(len(edges)):
        sl = slice(int(ptr[e]), int(ptr[e + 1]))
        front = pose.front_mask[sl]
        if est.status[e] != est.OK or pose.status[e] != pose.OK or not front.any() or planar[e]:
            continue
        median = float(np.median(pose.angle_deg[sl][front]))
        if min_angle < median < max_angle and median < best_median:
            best, best_median = e, median
    if best is None:
        return None, None, None, None, None
    sl = slice(int(ptr[best]), int(ptr[best + 1]))
    X = np.where(pose.front_mask[sl, None], pose.X[sl], np.nan)
    return best, pose.R[best].copy(), pose.t[best].copy(), X, pose.front_mask[sl].copy()


class DMatch:
    """One neighbour of ``knn_match``: the fields of cv2.DMatch that the reference reads (sfm.py:96), ``distance`` the
    float32 root of the squared distance."""
    __slots__ = ("queryIdx", "trainIdx", "distance", "imgIdx")

    def __init__(self, queryIdx, trainIdx, distance):
        self.queryIdx, self.trainIdx, self.distance, self.imgIdx = int(queryIdx), int(trainIdx), float(distance), 0

    def __repr__(self):
        return f"DMatch(queryIdx={self.queryIdx}, trainIdx={self.trainIdx}, distance={self.distance})"


def dmatch_lists(idx, dist_sq):
    """idx (n, 2), dist_sq (n, 2) of one edge -> what ``knnMatch(.., k=2)`` returns: per query the list of its neighbours
    that exist, nearest first."""
    root = np.sqrt(np.asarray(dist_sq, dtype=np.float64)).astype(np.float32)
    return [[DMatch(q, int(idx[q, k]), root[q, k]) for k in range(2) if idx[q, k] >= 0] for q in range(len(idx))]


def knn_match(query, train, k=2, device=0, backend=None):
    """The drop-in for ``cv2.BFMatcher(cv2.NORM_L2).knnMatch(query, train, k=2)`` (sfm.py:94): a list with, per query
    descriptor, the list of its two nearest train descriptors as :class:`DMatch`.  A train set with fewer than two rows
    gives empty lists."""
    if k != 2:
        raise ValueError("only k=2 is implemented")
    check_descriptors([query, train])
    be = backend if backend is not None else api.get_backend(device)
    be.set_descriptors([query, train])
    m = be.match_descriptors([(0, 1)])
    return dmatch_lists(m.idx, m.dist_sq)


def match_descriptors(descs, edges=None, ratio=0.5, form=0, profile=0, device=0, backend=None):
    """Lines 94-96 of ``SFM._match_features`` for a whole graph in one device call: ``descs`` a list of (n_i, D) arrays,
    ``edges`` (E, 2) of (query image, train image), None = all pairs u > v as the reference.  -> :class:`DescriptorMatches`;
    ``.pairs(e)`` is the reference's ``good_pairs`` of edge e."""
    _, ptr = check_descriptors(descs)
    check_match_edges(edges, len(ptr) - 1)
    check_match_options(ratio, form, profile)
    be = backend if backend is not None else api.get_backend(device)
    be.set_descriptors(descs)
    return be.match_descriptors(edges, ratio=ratio, form=form, profile=profile)


def match_features(descs, pts, K, min_matches=80, ratio=0.5, device=0, backend=None, **ransac_options):
    """The whole of ``SFM._match_features`` (sfm.py:88-107) in two device calls: every pair u > v matched with the ratio
    test, edges with at most 8 good pairs dropped, one :func:`Backend.fundamental_ransac` batch (``refit=1``) over the
    rest, edges with more than ``min_matches`` inliers kept.  ``descs``: list of (n_i, D); ``pts``: list of (n_i, 2) pixel
    positions of the same rows; the RANSAC defaults are those of :func:`find_fundamental_mat`.
    -> list of ``(u, v, inlier_pairs (k, 2) of (row in u, row in v), F, E = K^T F K)``."""
    _, ptr = check_descriptors(descs)
    rows = np.diff(ptr)
    pts = [np.asarray(p, dtype=np.float64) for p in pts]
    if len(pts) != len(rows):
        raise ValueError(f"{len(rows)} images have descriptors, {len(pts)} have pixels")
    for k, p in enumerate(pts):
        if p.shape != (rows[k], 2):
            raise ValueError(f"pixels of image {k} must be ({rows[k]}, 2), got {p.shape}")
    K = np.asarray(K, dtype=np.float64)
    if K.shape != (3, 3):
        raise ValueError("K must be (3, 3)")
    check_match_options(ratio)
    be = backend if backend is not None else api.get_backend(device)
    be.set_descriptors(descs)
    m = be.match_descriptors(None, ratio=ratio)
    cand = [(e, m.pairs(e)) for e in range(len(m.edges))]
    cand = [(e, gp) for e, gp in cand if len(gp) > 8]
    if not cand:
        return []
    p1 = [pts[m.edges[e, 0]][gp[:, 0]] for e, gp in cand]
    p2 = [pts[m.edges[e, 1]][gp[:, 1]] for e, gp in cand]
    eptr = np.concatenate([[0], np.cumsum([len(gp) for _, gp in cand])]).astype(np.int64)
    opts = dict(threshold=3.0, confidence=0.99, max_iters=1000, seed=0, refit=1)
    opts.update(ransac_options)
    est = be.fundamental_ransac(np.concatenate(p1), np.concatenate(p2), edge_ptr=eptr, **opts)
    out = []
    for k, (e, gp) in enumerate(cand):
        mask = est.inlier_mask[int(eptr[k]):int(eptr[k + 1])]
        if est.status[k] != est.OK or int(mask.sum()) <= min_matches:
            continue
        F = est.F_refit[k].copy()
        out.append((int(m.edges[e, 0]), int(m.edges[e, 1]), gp[mask], F, K.T @ F @ K))
    return out


def build_tracks(matches, n_features, device=0, backend=None, **options):
    """Feature tracks from the matched edges: what ``SFM._build_tracks`` (sfm.py:109-117) and the fusion bookkeeping of
    graph.py decide, as the connected components of the matches.  ``matches``: the list :func:`match_features` returns,
    ``(u, v, inlier_pairs, F, E)``, or plain ``(u, v, pairs)`` tuples, pairs (k, 2) of (row in u, row in v);
    ``n_features``: the number of features of every image.  Options as :meth:`Backend.build_tracks`.
    -> :class:`Tracks`; ``.problem(pts)`` gives the index arrays of ``set_problem``."""
    n_features = np.asarray(n_features)
    if n_features.ndim != 1 or (n_features.size and (not np.issubdtype(n_features.dtype, np.integer) or n_features.min() < 0)):
        raise ValueError("n_features must be a 1-D array of non-negative integers, one per image")
    img_ptr = np.concatenate([[0], np.cumsum(n_features, dtype=np.int64)]).astype(np.int64)
    matches = list(matches)
    for k, m in enumerate(matches):
        if len(m) < 3:
            raise ValueError(f"match {k} must be (u, v, pairs, ...)")
    edges = np.array([(int(m[0]), int(m[1])) for m in matches], dtype=np.int64).reshape(-1, 2)
    lists = [np.asarray(m[2]).reshape(-1, 2) if np.asarray(m[2]).size else np.empty((0, 2), dtype=np.int64) for m in matches]
    pair_ptr = np.concatenate([[0], np.cumsum([len(p) for p in lists], dtype=np.int64)]).astype(np.int64)
    pairs = np.concatenate(lists, axis=0) if lists else np.empty((0, 2), dtype=np.int64)
    args = check_track_inputs(img_ptr, edges, pair_ptr, pairs, None, **options)
    be = backend if backend is not None else api.get_backend(device)
    return be.build_tracks(*args[:5], **args[5])


class Reconstruction:
    """What :func:`reconstruct` returns.  ``registered`` (n_images, bool); ``cameras`` (n_images, 6): rotation vector and
    centre, the bundle-adjustment model's parameters, NaN where not registered; ``points`` (n_tracks, 3), NaN where
    unknown; ``known`` (n_tracks, bool); ``rounds``: one dict per round with ``tried`` and ``registered`` (image ids),
    ``failed`` (image -> why: the verdict of its resection, "few_views", "degenerate", "behind" or "high_error", or
    "absent" when none of its features lies in a track of the round's problem), ``points_added``, ``n_obs``
    (observations of the round's solve) and ``rmse_before`` / ``rmse_after`` of that solve (None when the round had no
    solve), with ``record_state=True`` also ``registered_before`` and ``known_before``, copies of the two masks the
    round started from; when images are left unregistered at the end, a closing entry that tried nothing and whose
    ``failed`` says "few_known" (fewer than ``min_known`` known tracks) or "not_grown" (its resection failed and the
    number of its known tracks has not grown since); ``tracks``: the :class:`Tracks`;
    ``problem()`` -> ``(x, args)`` of the final set, ``args`` the tuple of ``least_squares``, with ``cam_of`` / ``pt_of``
    (image id per camera, track id per point of that problem) and ``obs_feat`` as attributes."""

    def __init__(self, registered, cameras, points, known, rounds, tracks, x, args, cam_of, pt_of, obs_feat):
        self.registered, self.cameras, self.points, self.known = registered, cameras, points, known
        self.rounds, self.tracks = rounds, tracks
        self._x, self._args, self.cam_of, self.pt_of, self.obs_feat = x, args, cam_of, pt_of, obs_feat

    def problem(self):
        return self._x.copy(), self._args

    def transformed(self, s, R, t):
        """A new :class:`Reconstruction` in the frame ``X' = s R X + t``: ``cameras``, ``points`` and the ``x`` of
        ``problem()`` mapped by :func:`apply_similarity` (reprojections do not change), NaN rows staying NaN; masks,
        ``rounds``, ``tracks`` and the problem's ``args`` are shared with this one."""
        s, R, t = _similarity_args(s, R, t)
        cameras, points = _map_cameras(self.cameras, s, R, t), _map_points(self.points, s, R, t)
        x = apply_similarity(self._x, len(self.cam_of), s, R, t)
        return Reconstruction(self.registered.copy(), cameras, points, self.known.copy(), list(self.rounds), self.tracks, x,
                              self._args, self.cam_of, self.pt_of, self.obs_feat)

    def __repr__(self):
        return (f"Reconstruction(registered={int(self.registered.sum())}/{len(self.registered)}, "
                f"known={int(self.known.sum())}/{len(self.known)}, rounds={len(self.rounds)})")


# ---- similarities: one reconstruction against another, or against positions known from outside ----
def _similarity_args(s, R, t):
    s, R, t = float(s), np.asarray(R, dtype=np.float64), np.asarray(t, dtype=np.float64).reshape(-1)
    if R.shape != (3, 3) or t.shape != (3,):
        raise ValueError(f"R must be (3, 3) and t (3,), got {R.shape} and {t.shape}")
    return s, R, t


def _map_points(points, s, R, t):
    return s * (np.asarray(points, dtype=np.float64) @ R.T) + t


def _map_cameras(cameras, s, R, t):
    """(n, 6) rotation vector | centre under X' = s R X + t: the centre maps as a point, the rotation R_c becomes
    R_c R^T (x_cam = R_c (X - T) is then scaled by s, which a projection does not see); a NaN row stays NaN."""
    out = np.array(cameras, dtype=np.float64).reshape(-1, 6)
    for row in out:
        if np.isfinite(row).all():
            row[:3] = api._rotvec_from_matrix(api._matrix_from_rotvec(row[:3]) @ R.T)
    out[:, 3:] = _map_points(out[:, 3:], s, R, t)
    return out


def apply_similarity(x, n_cameras, s, R, t):
    """The parameter vector ``x`` (``n_cameras`` rows of rotation vector | centre, then the points) in the frame
    ``X' = s R X + t`` -> a new vector: points become ``s R X + t``, centres ``s R T + t``, rotations ``R_c R^T``, so every
    reprojection is what it was.  NumPy on the host: an elementwise map does not earn an upload, a launch and a
    download."""
    s, R, t = _similarity_args(s, R, t)
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    n = int(n_cameras)
    if n < 0 or 6 * n > x.shape[0] or (x.shape[0] - 6 * n) % 3:
        raise ValueError(f"x has {x.shape[0]} entries: not {n} cameras and whole points")
    return np.concatenate([_map_cameras(x[:6 * n].reshape(n, 6), s, R, t).ravel(),
                           _map_points(x[6 * n:].reshape(-1, 3), s, R, t).ravel()])


def _similarity_threshold(dst, threshold):
    """``threshold`` of the similarity calls; None: 0.02 x the median distance of the ``dst`` points from their
    coordinate-wise median (a convenience computed in NumPy: two per cent of the cloud's typical radius)."""
    if threshold is not None:
        return float(threshold)
    dst = np.asarray(dst, dtype=np.float64).reshape(-1, 3)
    if len(dst) == 0:
        return 1.0
    return 0.02 * float(np.median(np.linalg.norm(dst - np.median(dst, axis=0), axis=1)))


def estimate_similarity(src, dst, threshold=None, min_inliers=6, max_iters=1000, confidence=0.99, seed=0, refit=True,
                        pair_use=None, device=0, backend=None):
    """``dst ~ s R src + t`` between two (N, 3) point sets by RANSAC -> ``(s, R (3, 3), t (3,), mask (N,) bool)``: one call
    of :meth:`Backend.similarity_ransac`.  With ``refit=True`` the estimate over all inliers of the best hypothesis and ITS
    mask, else the best three-point hypothesis and its mask.  ``(None, None, None, mask)`` when the status is not OK or the
    mask holds fewer than ``min_inliers`` pairs: a triple whose two triangles happen to be similar fits its own similarity
    exactly (every triple of a mirrored copy does), so a handful of inliers says nothing.  ``threshold``: a distance in the units of ``dst``; None = 0.02 x the median distance of the used ``dst``
    points from their coordinate-wise median, a convenience computed in NumPy.  ``confidence`` only decides ``success``
    of the batch call; every one of the ``max_iters`` hypotheses is scored."""
    dst = np.asarray(dst, dtype=np.float64)
    used = dst.reshape(-1, 3) if pair_use is None else dst.reshape(-1, 3)[np.asarray(pair_use).ravel() != 0]
    be = backend if backend is not None else api.get_backend(device)
    est = be.similarity_ransac(src, dst, pair_use=pair_use, threshold=_similarity_threshold(used, threshold), confidence=confidence,
                               max_iters=max_iters, seed=seed, refit=1 if refit else 0)
    mask, count = (est.refit_mask, est.refit_inliers[0]) if refit else (est.inlier_mask, est.inliers[0])
    if est.status[0] != est.OK or count < int(min_inliers):
        return None, None, None, mask
    if refit:
        return float(est.scale_refit[0]), est.R_refit[0], est.t_refit[0], mask
    return float(est.scale[0]), est.R[0], est.t[0], mask


def _robust_similarity(be, src, dst, threshold, min_inliers, ransac, what):
    """The refit of one `similarity_ransac` over src -> dst, or ``ValueError`` naming ``what`` the pairs are."""
    if len(src) < int(min_inliers):
        raise ValueError(f"{len(src)} {what}: fewer than min_inliers = {int(min_inliers)}")
    ransac = dict(ransac)
    ransac["refit"] = 1
    est = be.similarity_ransac(src, dst, threshold=_similarity_threshold(dst, threshold), **ransac)
    if est.status[0] != est.OK or est.refit_inliers[0] < int(min_inliers):
        raise ValueError(f"no similarity with min_inliers = {int(min_inliers)} inliers among the {len(src)} {what} "
                         f"(status {int(est.status[0])}, {int(est.refit_inliers[0])} inliers)")
    return est


def align_reconstruction(rec, centres, threshold=None, min_inliers=6, device=0, backend=None, **ransac):
    """Put a :class:`Reconstruction` into the frame of camera positions known from outside (GPS, a survey, ground truth)
    -> ``(Reconstruction, SimilarityEstimate)``.  ``centres``: (n_images, 3), NaN rows where unknown; the correspondences
    are the registered images with a known position, camera centre -> position, in ascending image order (the estimate's
    masks run over them: ``np.flatnonzero(rec.registered & np.isfinite(centres).all(axis=1))``).  One
    :meth:`Backend.similarity_ransac` with ``refit=1`` (``ransac``: its other options; ``threshold`` as in
    :func:`estimate_similarity`), then :meth:`Reconstruction.transformed` by the refit.  ``ValueError`` when there are
    fewer than ``min_inliers`` correspondences, or fewer than ``min_inliers`` inliers."""
    centres = np.asarray(centres, dtype=np.float64)
    if centres.shape != (len(rec.registered), 3):
        raise ValueError(f"centres must be ({len(rec.registered)}, 3), got {centres.shape}")
    be = backend if backend is not None else api.get_backend(device)
    corr = rec.registered & np.isfinite(centres).all(axis=1)
    est = _robust_similarity(be, rec.cameras[corr, 3:6], centres[corr], threshold, min_inliers, ransac,
                             "registered images with a known position")
    return rec.transformed(est.scale_refit[0], est.R_refit[0], est.t_refit[0]), est


def merge_reconstructions(a, b, K, threshold=None, min_inliers=10, filter_options=None, device=0, backend=None, **ransac):
    """Join two reconstructions over the same :class:`Tracks` (say, two runs of :func:`reconstruct` from different
    ``init=`` pairs that each left images over) -> ``(Reconstruction, SimilarityEstimate)`` in a's frame.  Both must carry
    the ``Tracks`` of the last `build_tracks` on the back end, whose key points must be set (`reconstruct` leaves them so).
    The correspondences are the tracks known in both, b's point -> a's point, in ascending track order (the estimate's
    masks run over them); one :meth:`Backend.similarity_ransac` with ``refit=1`` (``ransac``: its other options;
    ``threshold`` as in :func:`estimate_similarity`, in a's units) maps b into a's frame.  ``registered`` and ``known``
    are the unions; where both have a camera or a point, a's is kept.  The problem is assembled with
    ``Backend.assemble_problem(registered, known, min_views=2)`` and one `reprojection_stats` pass with the trim's
    thresholds (``filter_options``: the keys and defaults of :func:`reconstruct`) prunes observations and points as the
    closing pass of `reconstruct` does.  NO solve is run: ``refine_reconstruction(*merged.problem())`` is the caller's
    next line.  Of ``a`` and ``b`` only ``registered``, ``cameras``, ``points``, ``known`` and ``tracks`` are read
    (observations that their own runs had dropped come back and face the closing pass again).  ``rounds`` of the result
    is ``a.rounds + b.rounds`` plus a closing dict with ``merged=True``, ``inliers`` and ``scale``.  ``ValueError`` for
    different tracks, fewer than ``min_inliers`` shared tracks or fewer than ``min_inliers`` inliers."""
    be = backend if backend is not None else api.get_backend(device)
    K = np.asarray(K, dtype=np.float64)
    if K.shape != (3, 3):
        raise ValueError("K must be (3, 3)")
    tracks = a.tracks
    if b.tracks is not tracks and not (b.tracks.n_tracks == tracks.n_tracks and np.array_equal(b.tracks.img_ptr, tracks.img_ptr) and
                                       np.array_equal(b.tracks.feat_track, tracks.feat_track)):
        raise ValueError("the two reconstructions do not carry the same tracks")
    n_images = len(tracks.img_ptr) - 1
    if getattr(be, "_plan_dims", None) != (n_images, tracks.n_tracks):
        raise ValueError("the reconstructions' tracks are not the result of the last build_tracks on this back end")
    thr = dict(max_error_px=4.0, min_depth=0.0, min_angle_deg=2.0, min_views=2)
    unknown = set(filter_options or {}) - set(thr)
    if unknown:
        raise TypeError(f"unknown filter option(s) {sorted(unknown)} (known: {sorted(thr)})")
    thr.update(filter_options or {})
    both = a.known & b.known
    est = _robust_similarity(be, b.points[both], a.points[both], threshold, min_inliers, ransac, "tracks known in both")
    s, R, t = _similarity_args(est.scale_refit[0], est.R_refit[0], est.t_refit[0])
    registered, known = a.registered | b.registered, a.known | b.known
    cameras = np.where(a.registered[:, None], a.cameras, _map_cameras(b.cameras, s, R, t))
    points = np.where(a.known[:, None], a.points, _map_points(b.points, s, R, t))
    cameras[~registered], points[~known] = np.nan, np.nan
    be.set_precision(64)
    sub = be.assemble_problem(registered, known, min_views=2)
    x, args, pt_of, obs_feat = sub.gather(cameras, points), sub.args(K), sub.pt_of, sub.obs_feat
    if len(obs_feat):
        be.set_fixed_cameras(())
        be.set_problem(*args)
        st = be.reprojection_stats(x, want=("obs", "points"), **thr)
        if st.n_obs_kept < st.n_obs or st.n_points_kept < args[1]:
            lost = pt_of[~st.pt_keep]
            known[lost], points[lost] = False, np.nan
            x, args, oi, pi = prune_problem(x, args, st.obs_keep, st.pt_keep)
            pt_of, obs_feat = pt_of[pi], obs_feat[oi]
    rounds = list(a.rounds) + list(b.rounds) + [dict(merged=True, inliers=int(est.refit_inliers[0]), scale=s)]
    return Reconstruction(registered, cameras, points, known, rounds, tracks, x, args, sub.cam_of, pt_of, obs_feat), est


_RESECT_VERDICTS = {1: "few_views", 2: "degenerate", 3: "behind", 4: "high_error"}


def _initial_edge(matches, pts, K, init, be, init_options=None):
    """-> (u, v, pts of u, pts of v, E) of the first pair: camera u at the identity, v from E's pose."""
    if init is None:
        index = select_initial_pair([(pts[m[0]][np.asarray(m[2])[:, 0]], pts[m[1]][np.asarray(m[2])[:, 1]]) for m in matches], K,
                                    backend=be, **dict(init_options or {}))[0]
        if index is None:
            raise ValueError("no edge qualifies as the initial pair (select_initial_pair)")
        init = (matches[index][0], matches[index][1])
    u, v = int(init[0]), int(init[1])
    for m in matches:
        if len(m) < 5:
            continue
        pairs = np.asarray(m[2]).reshape(-1, 2)
        if (int(m[0]), int(m[1])) == (u, v):
            return u, v, pts[u][pairs[:, 0]], pts[v][pairs[:, 1]], np.asarray(m[4], dtype=np.float64)
        if (int(m[0]), int(m[1])) == (v, u):                      # the same edge the other way round: x_u^T E^T x_v = 0
            return u, v, pts[u][pairs[:, 1]], pts[v][pairs[:, 0]], np.asarray(m[4], dtype=np.float64).T
    raise ValueError(f"init = ({u}, {v}) is no edge of `matches` with an essential matrix")


def reconstruct(matches, pts, K, tracks=None, init=None, batch=1, min_known=7, filter=True, fix_first=False, ftol=1e-10,
                ransac_options=None, triangulate_options=None, filter_options=None, filter_rounds=2, max_rounds=None,
                record_state=False, device=0, backend=None, init_options=None, robust_triangulation=False):
    """Incremental reconstruction, the loop of ``SFM.construct`` (sfm.py:59-71, 182-241) camera by camera on one
    :class:`Backend`: `plan_views` chooses the next images, `assemble_problem` cuts the growing problem out of the tracks,
    `resect_ransac` registers, `triangulate` adds points, bundle adjustment and (``filter=True``)
    :func:`refine_reconstruction` clean up.  DESIGN.md section 25.

    ``matches``: what :func:`match_features` returns, ``(u, v, pairs, F, E)``; ``pts``: list of (n_i, 2) pixel arrays;
    ``tracks``: the :class:`Tracks` of the last `build_tracks` on ``backend`` over these matches (None: built here);
    ``init``: ``(u, v)``, an edge of ``matches`` -- u is put at the identity, v at the pose of the edge's ``E`` -- or None:
    :func:`select_initial_pair`, with the keywords of the dict ``init_options`` when that is given (for instance
    ``dict(max_homography_ratio=0.8)``; None: its defaults, as before).  Every round takes the ``batch`` best unregistered images (0 = all) that see at least
    ``min_known`` known tracks (7: the reference's ``> 6``); an image whose resection failed is tried again only after
    that number has grown.  An observation of a new camera that its RANSAC pose leaves out is dropped for good, and a
    new point must triangulate within ``max_error_px`` of the trim (unless ``triangulate_options`` says otherwise).
    ``ransac_options``, ``triangulate_options``: fields of the two calls' option structures;
    ``filter_options``: ``max_error_px`` (4), ``min_depth`` (0), ``min_angle_deg`` (2), ``min_views`` (2) of the trim
    and of the final pass; ``fix_first=True`` holds camera u still in every solve (the reference holds nothing).
    ``robust_triangulation=True``: the rounds add points with `triangulate_ransac` -- a track with a wrong observation
    comes back with its point and that observation is dropped for good, as after `resect_ransac`, where `triangulate`
    would refuse the whole track round after round; ``triangulate_options`` may then name the fields of
    ``sfmba_tri_ransac_options`` as well, and ``threshold`` defaults to ``max_error_px`` of the trim (4 without one).
    -> :class:`Reconstruction`."""
    be = backend if backend is not None else api.get_backend(device)
    K = np.asarray(K, dtype=np.float64)
    if K.shape != (3, 3):
        raise ValueError("K must be (3, 3)")
    if int(batch) != batch or batch < 0:
        raise ValueError(f"batch must be a non-negative integer, got {batch!r}")
    matches = list(matches)
    pts = [np.ascontiguousarray(p, dtype=np.float64).reshape(-1, 2) for p in pts]
    n_images = len(pts)
    ransac_options, triangulate_options = dict(ransac_options or {}), dict(triangulate_options or {})
    thr = dict(max_error_px=4.0, min_depth=0.0, min_angle_deg=2.0, min_views=2)
    unknown = set(filter_options or {}) - set(thr)
    if unknown:
        raise TypeError(f"unknown filter option(s) {sorted(unknown)} (known: {sorted(thr)})")
    thr.update(filter_options or {})
    if not filter:
        thr = dict(max_error_px=np.inf, min_depth=-np.inf, min_angle_deg=0.0, min_views=0)
    # a new point must pass the pixel threshold of the trim as well: bundle adjustment is a plain least squares, and
    # one track with a wrong observation bends the cameras until good observations fail the trim that follows it
    triangulate_options.setdefault("max_error_px", thr["max_error_px"])
    robust_options = None
    if robust_triangulation:
        robust_options = dict(triangulate_options)
        robust_options.setdefault("threshold", thr["max_error_px"] if np.isfinite(thr["max_error_px"]) else 4.0)
        plain = {f[0] for f in _capi.TriangulateOptions._fields_}
        triangulate_options = {k: v for k, v in triangulate_options.items() if k in plain}      # (the initial pair's call)
    if tracks is None:
        tracks = build_tracks(matches, [len(p) for p in pts], backend=be)
    elif getattr(be, "_plan_dims", None) != (n_images, tracks.n_tracks):
        raise ValueError("`tracks` is not the result of the last build_tracks on this back end")
    if len(tracks.img_ptr) - 1 != n_images or any(len(p) != n for p, n in zip(pts, np.diff(tracks.img_ptr))):
        raise ValueError("`pts` does not have the tracks' number of features per image")
    be.set_keypoints(pts)
    be.set_precision(64)
    n_tracks, N = tracks.n_tracks, int(tracks.img_ptr[-1])
    registered, known = np.zeros(n_images, dtype=bool), np.zeros(n_tracks, dtype=bool)
    cameras, points = np.full((n_images, 6), np.nan), np.full((n_tracks, 3), np.nan)
    feat_ok = np.ones(N, dtype=bool)                             # False: the observation of this feature was dropped for good
    all_tracks = np.ones(n_tracks, dtype=bool)
    rounds = []

    def start(sub):                                              # the sub-problem on the handle, and its parameter vector
        be.set_fixed_cameras(())
        be.set_problem(*sub.args(K))
        return np.nan_to_num(sub.gather(cameras, points), nan=0.0)

    def take_points(sub, tri):
        new = sub.pt_of[tri.ok]
        points[new], known[new] = tri.points[tri.ok], True
        return len(new)

    # ---- the initial pair
    u, v, p1, p2, E = _initial_edge(matches, pts, K, init, be, init_options)
    pose = be.recover_pose(E, p1, p2, K)
    if pose.status[0] != pose.OK:                                # (a TIE is no start for a reconstruction: select_initial_pair)
        raise ValueError(f"the pose of the initial pair ({u}, {v}) could not be recovered (status {int(pose.status[0])})")
    R, t = pose.R[0].reshape(3, 3), pose.t[0].reshape(3)
    cameras[u] = 0.0
    cameras[v] = np.concatenate([api._rotvec_from_matrix(R), -R.T @ t])
    registered[[u, v]] = True
    sub = be.assemble_problem(registered, all_tracks, min_views=2)
    if sub.n_obs == 0:
        raise ValueError(f"images {u} and {v} share no track")
    take_points(sub, be.triangulate(start(sub), **triangulate_options))

    # ---- the rounds
    tried_known = np.full(n_images, -1, dtype=np.int64)          # img_known at an image's last failed resection
    for _ in range(int(max_rounds) if max_rounds is not None else 2 * n_images + 2):
        plan = be.plan_views(registered, known)
        cand = plan.candidates(min_known)
        cand = cand[plan.img_known[cand] > tried_known[cand]]
        if batch:
            cand = cand[:int(batch)]
        if len(cand) == 0:
            left = np.flatnonzero(~registered)
            if len(left):
                rounds.append(dict(tried=[], registered=[], points_added=0, n_obs=0, rmse_before=None, rmse_after=None,
                                   failed={int(i): "few_known" if plan.img_known[i] < min_known else "not_grown" for i in left}))
            break
        use = registered.copy()
        use[cand] = True
        sub = be.assemble_problem(use, all_tracks, min_views=2)
        x = start(sub)
        obs_ok = feat_ok[sub.obs_feat]
        resect_use = known[sub.pt_of][sub.point_indices] & obs_ok
        rr = be.resect_ransac(x, select=np.isin(sub.cam_of, cand), obs_use=resect_use, **ransac_options)
        info = dict(tried=[int(i) for i in cand], registered=[], failed={}, points_added=0, n_obs=0, rmse_before=None,
                    rmse_after=None)
        if record_state:
            info["registered_before"], info["known_before"] = plan.cam_reg.copy(), plan.trk_known.copy()
        position = {int(i): c for c, i in enumerate(sub.cam_of)}
        for i in (int(i) for i in cand):
            c = position.get(i)
            if c is not None and rr.ok[c]:
                cameras[i], registered[i] = rr.cameras[c], True
                info["registered"].append(i)
            else:
                tried_known[i] = plan.img_known[i]
                info["failed"][i] = "absent" if c is None else _RESECT_VERDICTS.get(int(rr.status[c]), str(int(rr.status[c])))
        rounds.append(info)
        if not info["registered"]:
            break
        # what a new camera's pose does not agree with is a wrong 2-D--3-D match: dropped for good
        new_cam = np.isin(sub.cam_of, info["registered"])
        feat_ok[sub.obs_feat[resect_use & new_cam[sub.camera_indices] & ~rr.inlier_mask]] = False
        obs_ok = feat_ok[sub.obs_feat]
        x = np.nan_to_num(sub.gather(cameras, points), nan=0.0)
        if robust_triangulation:
            tri_use = registered[sub.cam_of][sub.camera_indices] & obs_ok
            tri = be.triangulate_ransac(x, select=~known[sub.pt_of], obs_use=tri_use, **robust_options)
            # what the point of a new track does not agree with is a wrong match in the track: dropped for good
            feat_ok[sub.obs_feat[tri_use & tri.ok[sub.point_indices] & ~tri.inlier_mask]] = False
        else:
            tri = be.triangulate(x, select=~known[sub.pt_of], obs_use=registered[sub.cam_of][sub.camera_indices] & obs_ok,
                                 **triangulate_options)
        info["points_added"] = take_points(sub, tri)
        # bundle adjustment over the registered cameras and the known tracks, without the observations dropped so far
        x, args, cam_of, pt_of, obs_feat = _final_set(be, registered, known, feat_ok, cameras, points, K)
        info["n_obs"] = len(obs_feat)
        for k in range(max(int(filter_rounds), 1) if filter else 1):
            kw = dict(ftol=ftol)
            if fix_first:
                kw["jac_sparsity"] = api.create_sparsity_matrix(args[0], args[1], len(obs_feat), args[2], args[3],
                                                                fixed_camera_indices=(int(np.flatnonzero(cam_of == u)[0]),))
            if not filter:
                result = api.least_squares(api.compute_residuals, x, x_scale="jac", method="trf", args=args, backend=be, **kw)
                x = result.x
            else:
                pidx = np.asarray(args[3])
                result, (x, args), (oi, pi), _ = refine_reconstruction(x, args, rounds=1, backend=be, **thr, **kw)
                lost_pt = np.ones(len(pt_of), dtype=bool)
                lost_pt[pi] = False
                lost_obs = np.ones(len(obs_feat), dtype=bool)
                lost_obs[oi] = False
                # an observation that went while its point stayed failed its own test: dropped for good; a track
                # that went loses its point and may be triangulated again
                feat_ok[obs_feat[lost_obs & ~lost_pt[pidx]]] = False
                known[pt_of[lost_pt]] = False
                points[pt_of[lost_pt]] = np.nan
                pt_of, obs_feat = pt_of[pi], obs_feat[oi]
            if k == 0:
                info["rmse_before"] = float(result.rmse0)
            info["rmse_after"] = float(result.rmse)
            if not filter or not (lost_pt.any() or lost_obs.any()):
                break
        cameras[cam_of] = x[:6 * len(cam_of)].reshape(-1, 6)
        points[pt_of] = x[6 * len(cam_of):].reshape(-1, 3)

    # ---- what the result contains: one statistics pass with the same thresholds
    x, args, cam_of, pt_of, obs_feat = _final_set(be, registered, known, feat_ok, cameras, points, K)
    if len(obs_feat):
        be.set_fixed_cameras(())
        be.set_problem(*args)
        st = be.reprojection_stats(x, want=("obs", "points"), **thr)
        if st.n_obs_kept < st.n_obs or st.n_points_kept < args[1]:
            lost = pt_of[~st.pt_keep]
            known[lost], points[lost] = False, np.nan
            x, args, oi, pi = prune_problem(x, args, st.obs_keep, st.pt_keep)
            pt_of, obs_feat = pt_of[pi], obs_feat[oi]
    return Reconstruction(registered, cameras, points, known, rounds, tracks, x, args, cam_of, pt_of, obs_feat)


def _final_set(be, registered, known, feat_ok, cameras, points, K):
    """The problem over the registered cameras and the known tracks without the dropped observations ->
    ``(x, args, cam_of, pt_of, obs_feat)``; a track left with fewer than two observations goes (its point stays known)."""
    sub = be.assemble_problem(registered, known, min_views=2)
    x, args = sub.gather(cameras, points), sub.args(K)
    keep = feat_ok[sub.obs_feat]
    if keep.all():
        return x, args, sub.cam_of, sub.pt_of, sub.obs_feat
    pt_keep = np.bincount(sub.point_indices[keep], minlength=sub.n_points) >= 2
    x, args, oi, pi = prune_problem(x, args, keep, pt_keep)
    return x, args, sub.cam_of, sub.pt_of[pi], sub.obs_feat[oi]


def load_calibration_data(txt_path):
    """3x3 whitespace-separated text -> ndarray, /root/reference/sfm_lite/utils.py:24-35."""
    K = np.array([[float(v) for v in line.split()] for line in open(txt_path) if line.strip()])
    assert K.shape == (3, 3), K.shape
    return K


def save_problem(path, x0, n_cameras, n_points, camera_indices, point_indices, points_2d, K):
    """The arguments of the reference's least_squares call as one .npz (no pickles)."""
    np.savez_compressed(path, x0=np.asarray(x0, dtype=np.float64), dims=np.array([n_cameras, n_points], dtype=np.int64),
                        camera_indices=np.asarray(camera_indices, dtype=np.int64),
                        point_indices=np.asarray(point_indices, dtype=np.int64), points_2d=np.asarray(points_2d),
                        K=np.asarray(K, dtype=np.float64))


def load_problem(path):
    """-> (x0, args) with args the tuple of sfm.py:268."""
    g = np.load(path, allow_pickle=False)
    C, P = (int(v) for v in g["dims"])
    return g["x0"], (C, P, g["camera_indices"], g["point_indices"], g["points_2d"], g["K"])
