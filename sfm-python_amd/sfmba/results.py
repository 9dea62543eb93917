"""What the calls of `Backend` return: plain holders of the arrays a call filled."""
from __future__ import annotations

import dataclasses

import numpy as np


class _PairEstimate:
    """What the pair-RANSAC estimates have in common, from the outputs of `Backend._pair_ransac` by name: the status
    codes, ``inlier_mask``, ``inliers``, ``best``, ``success``, ``status``, ``hyp_inliers``, ``n_ok``, ``kernel_us`` and
    the batch's ``edge_ptr`` (``set_ptr`` for a batch of sets)."""

    OK, FEW_PAIRS, DEGENERATE = 0, 1, 2
    _batch = "edge"

    def __init__(self, out):
        self.inlier_mask, self.inliers, self.best = out["inlier_mask"], out["inliers"], out["best"]
        self.success, self.status, self.hyp_inliers = out["success"], out["status"], out["hyp_inliers"]
        self.n_ok, self.kernel_us = int(out["n_ok"]), float(out["kernel_us"])
        setattr(self, f"{self._batch}_ptr", out["ptr"])

    @property
    def ok(self):
        return self.status == self.OK

    def __repr__(self):
        return f"{type(self).__name__}(n_{self._batch}s={len(self.status)}, n_ok={self.n_ok})"


class FundamentalEstimate(_PairEstimate):
    """What `Backend.fundamental_ransac` returns (include/sfmba.h: sfmba_fundamental_ransac), per edge of the batch:
    ``F`` and ``F_refit`` (E, 3, 3), unit Frobenius norm, largest entry positive (``F_refit`` equals ``F`` unless
    ``refit=1``); ``inliers``, ``best`` (the winning hypothesis), ``status`` (one of ``OK, FEW_PAIRS, DEGENERATE``) as
    int32 (E), ``success`` (E, bool): inliers / used pairs >= confidence; ``inlier_mask`` (M, bool) over the stored pairs;
    ``hyp_inliers`` (E, H) the count of every hypothesis, or None when not asked for; ``n_ok``; ``kernel_us``
    (``profile=1``, else 0)."""

    def __init__(self, out):
        super().__init__(out)
        self.F, self.F_refit = out["F"], out["F_refit"]


class HomographyEstimate(_PairEstimate):
    """What `Backend.homography_ransac` returns (include/sfmba.h: sfmba_homography_ransac), per edge of the batch:
    ``H`` and ``H_refit`` (E, 3, 3), ``x2 ~ H x1``, unit Frobenius norm, largest entry positive (``H_refit`` equals ``H``
    unless ``refit=1``); ``inliers``, ``refit_inliers``, ``best`` (the winning hypothesis), ``status`` (one of ``OK,
    FEW_PAIRS, DEGENERATE``) as int32 (E), ``success`` (E, bool): inliers / used pairs >= confidence; ``inlier_mask`` (of
    ``H``) and ``refit_mask`` (of ``H_refit``) (M, bool) over the stored pairs; ``hyp_inliers`` (E, H) the count of every
    hypothesis, or None when not asked for; ``n_ok``; ``kernel_us`` (``profile=1``, else 0)."""

    def __init__(self, out):
        super().__init__(out)
        self.H, self.H_refit, self.refit_mask, self.refit_inliers = out["H"], out["H_refit"], out["refit_mask"], out["refit_inliers"]


class SimilarityEstimate(_PairEstimate):
    """What `Backend.similarity_ransac` returns (include/sfmba.h: sfmba_similarity_ransac), per set of the batch:
    ``dst ~ scale R src + t`` with ``scale`` (E), ``R`` (E, 3, 3), ``t`` (E, 3) of the best hypothesis and ``scale_refit``,
    ``R_refit``, ``t_refit`` of the estimate over all its inliers (copies unless ``refit=1``); ``inliers``,
    ``refit_inliers``, ``best`` (the winning hypothesis), ``status`` (one of ``OK, FEW_PAIRS, DEGENERATE``) as int32 (E),
    ``success`` (E, bool): inliers / used pairs >= confidence; ``inlier_mask`` (of the best hypothesis) and ``refit_mask``
    (of the refit) (M, bool) over the stored pairs; ``hyp_inliers`` (E, H) the count of every hypothesis, or None when not
    asked for; ``n_ok``; ``kernel_us`` (``profile=1``, else 0); ``set_ptr``.  A status OK says only that three or more
    pairs agree: how many inliers are enough is the caller's decision."""

    _batch = "set"

    def __init__(self, out):
        super().__init__(out)
        sim, sim_refit = out["sim"], out["sim_refit"]
        self.scale, self.R, self.t = sim[:, 0].copy(), sim[:, 1:10].reshape(-1, 3, 3).copy(), sim[:, 10:13].copy()
        self.scale_refit, self.R_refit, self.t_refit = (sim_refit[:, 0].copy(), sim_refit[:, 1:10].reshape(-1, 3, 3).copy(),
                                                        sim_refit[:, 10:13].copy())
        self.refit_mask, self.refit_inliers = out["refit_mask"], out["refit_inliers"]


class EssentialEstimate(_PairEstimate):
    """What `Backend.essential_ransac` returns (include/sfmba.h: sfmba_essential_ransac), per edge of the batch: ``E``
    (n_edges, 3, 3), unit Frobenius norm, largest entry positive (compare up to sign); ``inliers``, ``best`` (the winning
    hypothesis), ``best_root`` (its candidate, by ascending z), ``status`` (one of ``OK, FEW_PAIRS, DEGENERATE``) as int32
    (n_edges), ``success`` (n_edges, bool): inliers / used pairs >= confidence; ``inlier_mask`` (M, bool) over the stored
    pairs; ``hyp_inliers`` and ``hyp_roots`` (n_edges, H) the count and the number of real roots of every hypothesis, or
    None when not asked for; ``n_ok``; ``kernel_us`` (``profile=1``, else 0)."""

    def __init__(self, out):
        super().__init__(out)
        self.E, self.best_root, self.hyp_roots = out["E"], out["best_root"], out["hyp_roots"]


class RelativePose:
    """What `Backend.recover_pose` returns (include/sfmba.h: sfmba_recover_pose), per edge: ``R`` (E, 3, 3) and ``t``
    (E, 3), ``x2 = R x1 + t`` with ``|t| = 1``; ``front`` (E) the winner's pairs in front, ``front_all`` (E, 4) every
    candidate's; ``sum_err`` (E) the reference's reprojection total; ``status`` (E) one of ``OK, FEW_PAIRS, DEGENERATE,
    TIE``; per stored pair ``front_mask`` (M, bool), ``X`` (M, 3) and ``angle_deg`` (M), NaN where a pair took no part /
    is not in front; ``n_ok``; ``kernel_us``."""

    OK, FEW_PAIRS, DEGENERATE, TIE = 0, 1, 2, 3

    def __init__(self, R, t, front_mask, X, angle_deg, front, front_all, sum_err, status, n_ok, kernel_us, edge_ptr):
        self.R, self.t, self.front_mask, self.X, self.angle_deg = R, t, front_mask, X, angle_deg
        self.front, self.front_all, self.sum_err, self.status = front, front_all, sum_err, status
        self.n_ok, self.kernel_us, self.edge_ptr = int(n_ok), float(kernel_us), edge_ptr

    @property
    def ok(self):
        return self.status == self.OK

    def __repr__(self):
        return f"RelativePose(n_edges={len(self.status)}, n_ok={self.n_ok})"



class DescriptorMatches:
    """What `Backend.match_descriptors` returns (include/sfmba.h: sfmba_match_descriptors).  Per query row, the edges'
    query images one after another (edge e owns ``query_ptr[e]:query_ptr[e + 1]``): ``idx`` (Q, 2) int32 the nearest and
    second nearest train row (-1: none), ``dist_sq`` (Q, 2) their squared L2 distances (+inf: none), ``good`` (Q, bool)
    Lowe's ratio test.  Per edge: ``edge_good`` the number of good queries, ``edge_status`` (``OK`` or ``FEW``: a train
    image with fewer than two rows or an empty query image).  ``edges`` (E, 2) the batch; ``n_ok``; ``kernel_us``
    (``profile=1``, else 0)."""

    OK, FEW = 0, 1

    def __init__(self, edges, query_ptr, idx, dist_sq, good, edge_good, edge_status, n_ok, kernel_us):
        self.edges, self.query_ptr, self.idx, self.dist_sq, self.good = edges, query_ptr, idx, dist_sq, good
        self.edge_good, self.edge_status, self.n_ok, self.kernel_us = edge_good, edge_status, int(n_ok), float(kernel_us)

    def pairs(self, e):
        """(k, 2) int array of (query index, train index) of the good queries of edge ``e`` in ascending query order:
        the reference's ``good_pairs`` (sfm.py:96)."""
        b, n = int(self.query_ptr[e]), int(self.query_ptr[e + 1])
        q = np.flatnonzero(self.good[b:n])
        return np.stack([q, self.idx[b:n, 0][q]], axis=1).astype(int)

    def __repr__(self):
        return f"DescriptorMatches(n_edges={len(self.edge_status)}, n_ok={self.n_ok})"



class Tracks:
    """What `Backend.build_tracks` returns (include/sfmba.h: sfmba_build_tracks): the connected components of the used
    match pairs.  ``feat_track`` (N) int32 per global feature id: its track, or ``UNMATCHED`` (in no used pair), ``SHORT``
    (its component failed a length test), ``CONFLICT`` (its component holds two features of one image and was dropped).
    The kept tracks as a CSR in point-major order: track t owns ``track_ptr[t]:track_ptr[t + 1]`` of ``track_feat``
    (global feature ids, ascending), ``track_image`` and ``track_row`` (the row within the image).  ``counts``: a dict
    of ``components``, ``tracks``, ``short``, ``long``, ``conflict``, ``observations``; ``n_tracks``; ``kernel_us``
    (``profile=1``, else 0); ``img_ptr`` the input's."""

    UNMATCHED, SHORT, CONFLICT = -1, -2, -3
    COUNTS = ("components", "tracks", "short", "long", "conflict", "observations")

    def __init__(self, img_ptr, feat_track, track_ptr, track_feat, track_image, counts, kernel_us):
        self.img_ptr, self.feat_track, self.track_ptr = img_ptr, feat_track, track_ptr
        self.track_feat, self.track_image = track_feat, track_image
        self.track_row = (track_feat - img_ptr[track_image]).astype(np.int32)
        self.counts = {k: int(v) for k, v in zip(self.COUNTS, counts)}
        self.n_tracks, self.kernel_us = len(track_ptr) - 1, float(kernel_us)

    def track_of(self, image, row):
        """The track of feature ``row`` of ``image`` (or one of the negative states); arrays are taken element-wise."""
        image, row = np.asarray(image), np.asarray(row)
        if np.any(image < 0) or np.any(image >= len(self.img_ptr) - 1):
            raise ValueError("image out of range")
        if np.any(row < 0) or np.any(row >= self.img_ptr[image + 1] - self.img_ptr[image]):
            raise ValueError("row outside its image")
        t = self.feat_track[self.img_ptr[image] + row]
        return int(t) if t.ndim == 0 else t

    def problem(self, pts):
        """The index arrays of a bundle-adjustment problem over the kept tracks: ``pts`` a list of (n_i, 2) pixel positions
        of the images' features -> ``(n_points, camera_indices, point_indices, points_2d)`` with camera index = image id
        and point index = track id, point-major as `set_problem` prefers."""
        rows = np.diff(self.img_ptr)
        if len(pts) != len(rows):
            raise ValueError(f"{len(rows)} images, {len(pts)} pixel arrays")
        pts = [np.asarray(p, dtype=np.float64).reshape(-1, 2) for p in pts]
        for k, a in enumerate(pts):
            if a.shape[0] != rows[k]:
                raise ValueError(f"pixels of image {k} must be ({rows[k]}, 2), got {a.shape}")
        allpts = np.concatenate(pts, axis=0) if pts else np.empty((0, 2))
        point_indices = np.repeat(np.arange(self.n_tracks, dtype=np.int32), np.diff(self.track_ptr))
        return self.n_tracks, self.track_image.copy(), point_indices, np.ascontiguousarray(allpts[self.track_feat])

    def __repr__(self):
        return f"Tracks(n_tracks={self.n_tracks}, observations={self.counts['observations']})"



class ViewPlan:
    """What `Backend.plan_views` returns (include/sfmba.h: sfmba_plan_views): the counts a view selection needs.
    ``cam_reg`` (n_images, bool) and ``trk_known`` (n_tracks, bool): the masks given; ``trk_reg_views`` (n_tracks, int32)
    registered images among a track's views; ``img_tracks``, ``img_known``, ``img_gain`` (n_images, int32): an image's
    features in a kept track, those of a known track (``len(feat2point_index)`` of graph.py:46-54), and those of an
    unknown track that another registered image sees; ``totals``: a dict of ``registered`` images, ``known`` tracks and
    tracks ``ready`` to be triangulated (unknown, two registered views or more); ``kernel_us`` (``profile=1``, else 0)."""

    def __init__(self, cam_reg, trk_known, trk_reg_views, img_tracks, img_known, img_gain, totals, kernel_us):
        self.cam_reg, self.trk_known, self.trk_reg_views = cam_reg, trk_known, trk_reg_views
        self.img_tracks, self.img_known, self.img_gain = img_tracks, img_known, img_gain
        self.totals = dict(zip(("registered", "known", "ready"), (int(v) for v in totals)))
        self.kernel_us = float(kernel_us)

    def candidates(self, min_known=7):
        """The unregistered images with ``img_known >= min_known``, by ``img_known`` descending, ties to the lower id."""
        idx = np.flatnonzero(~self.cam_reg & (self.img_known >= min_known))
        return idx[np.lexsort((idx, -self.img_known[idx].astype(np.int64)))]

    def edge_scores(self, edges, n_pairs):
        """``min(img_known[u], img_known[v]) / n_pairs`` for ``edges`` (E, 2): the score of ``_select_edge`` (sfm.py:195)
        with the known tracks of the transitive closure in place of ``Node.pts3d_pts2d``."""
        edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
        n_pairs = np.asarray(n_pairs, dtype=np.float64).reshape(-1)
        if n_pairs.shape[0] != edges.shape[0]:
            raise ValueError(f"{edges.shape[0]} edges, {n_pairs.shape[0]} pair counts")
        return np.minimum(self.img_known[edges[:, 0]], self.img_known[edges[:, 1]]) / n_pairs

    def __repr__(self):
        return f"ViewPlan({', '.join(f'{k}={v}' for k, v in self.totals.items())})"


class SubProblem:
    """What `Backend.assemble_problem` returns (include/sfmba.h: sfmba_assemble_problem, sfmba_get_assembled): the
    bundle-adjustment problem over a set of images and tracks.  ``cam_of`` (n_cameras, int32) image id per camera and
    ``pt_of`` (n_points, int32) track id per point, both ascending; ``camera_indices``, ``point_indices`` (n_obs, int64)
    renumbered through them; ``obs_feat`` (n_obs, int32) global feature ids; ``points_2d`` (n_obs, 2) their pixels, or
    None when the back end holds no keypoints; point-major, ascending by feature id within a point.  ``counts``: a dict
    of ``cameras``, ``points``, ``observations``; ``kernel_us`` (``profile=1``, else 0)."""

    def __init__(self, cam_of, pt_of, camera_indices, point_indices, obs_feat, points_2d, kernel_us):
        self.cam_of, self.pt_of, self.camera_indices, self.point_indices = cam_of, pt_of, camera_indices, point_indices
        self.obs_feat, self.points_2d, self.kernel_us = obs_feat, points_2d, float(kernel_us)
        self.n_cameras, self.n_points, self.n_obs = len(cam_of), len(pt_of), len(obs_feat)
        self.counts = dict(cameras=self.n_cameras, points=self.n_points, observations=self.n_obs)

    def args(self, K):
        """The tuple of `set_problem` and of ``least_squares(..., args=)``."""
        if self.points_2d is None:
            raise ValueError("the sub-problem has no pixels: call set_keypoints before assemble_problem")
        return (self.n_cameras, self.n_points, self.camera_indices, self.point_indices, self.points_2d, K)

    def gather(self, cameras, points):
        """``cameras`` (n_images, 6) and ``points`` (n_tracks, 3) -> the parameter vector ``x`` of the sub-problem."""
        cameras, points = np.asarray(cameras, dtype=np.float64), np.asarray(points, dtype=np.float64)
        return np.concatenate([cameras[self.cam_of].ravel(), points[self.pt_of].ravel()])

    def scatter(self, x, cameras, points):
        """The cameras and points of ``x`` written back into ``cameras`` (n_images, 6) and ``points`` (n_tracks, 3)."""
        x = np.asarray(x, dtype=np.float64).ravel()
        if x.shape[0] != 6 * self.n_cameras + 3 * self.n_points:
            raise ValueError(f"x has {x.shape[0]} entries, expected {6 * self.n_cameras + 3 * self.n_points}")
        cameras[self.cam_of] = x[:6 * self.n_cameras].reshape(-1, 6)
        points[self.pt_of] = x[6 * self.n_cameras:].reshape(-1, 3)

    def __repr__(self):
        return f"SubProblem(cameras={self.n_cameras}, points={self.n_points}, observations={self.n_obs})"



class ReprojectionStats:
    """What `Backend.reprojection_stats` returns (include/sfmba.h: sfmba_reprojection_stats).  Arrays that were not asked
    for are None.  ``obs_*`` (N) in the caller's observation order, ``pt_*`` (P), ``cam_*`` (C); the summary's fields
    ``n_obs, n_obs_kept, n_points_kept, n_behind, sum_err, sum_err2, max_err`` run over the finally kept observations."""

    _ARRAYS = ("obs_err", "obs_depth", "obs_keep", "pt_views", "pt_max_err", "pt_sum_err2", "pt_min_depth",
               "pt_max_angle_deg", "pt_keep", "cam_views", "cam_sum_err", "cam_max_err", "cam_behind")
    _SUMMARY = ("n_obs", "n_obs_kept", "n_points_kept", "n_behind", "sum_err", "sum_err2", "max_err")

    def __init__(self, arrays, summary):
        for name in self._ARRAYS:
            setattr(self, name, arrays.get(name))
        for name in self._SUMMARY:
            v = getattr(summary, name)
            setattr(self, name, float(v) if isinstance(v, float) else int(v))

    @property
    def mean_error_px(self):
        """Mean reprojection error over the kept observations (0 when none is kept)."""
        return self.sum_err / max(self.n_obs_kept, 1)

    @property
    def rms_error_px(self):
        """sqrt(mean err^2) over the kept observations."""
        return float(np.sqrt(self.sum_err2 / max(self.n_obs_kept, 1)))

    @property
    def cam_mean_err(self):
        if self.cam_sum_err is None:
            return None
        return self.cam_sum_err / np.maximum(self.cam_views, 1)

    def summary(self):
        d = {name: getattr(self, name) for name in self._SUMMARY}
        d["mean_error_px"], d["rms_error_px"] = self.mean_error_px, self.rms_error_px
        return d

    def __repr__(self):
        return "ReprojectionStats(" + ", ".join(f"{k}={v!r}" for k, v in self.summary().items()) + ")"


class Covariance:
    """What `Backend.covariance` returns (include/sfmba.h: sfmba_covariance).  ``cam_cov`` (C,6,6), ``cam_full`` (6C,6C) or
    None, ``cam_sigma`` (C,2), ``pt_cov`` (P,3,3) / ``pt_sigma`` (P) or None, ``pt_status`` (P: 0 fine, 1 undetermined,
    3 no observation), ``held`` (6C: 0 free, 1 held, 2 unobserved), ``sigma2``, ``dof``, ``cost``, ``status`` (0 fine, 1
    rank deficient cameras, 2 undetermined points), ``gauge`` = (g0, g1, axis) of the default gauge or -1s, ``bad_param``,
    ``n_bad_points``, ``bad_point``, ``min_pivot_rel``, ``kernel_us``.  After a rank failure every matrix is NaN."""

    STATUS = {0: "ok", 1: "rank deficient", 2: "undetermined points"}

    def __init__(self, arrays, info):
        for name in ("cam_cov", "cam_full", "cam_sigma", "pt_cov", "pt_sigma", "pt_status", "held"):
            setattr(self, name, arrays.get(name))
        self.sigma2, self.cost, self.dof, self.status = float(info.sigma2), float(info.cost), int(info.dof), int(info.status)
        self.gauge = (int(info.g0), int(info.g1), int(info.g1_axis))
        self.n_free, self.n_held, self.bad_param = int(info.n_free), int(info.n_held), int(info.bad_param)
        self.n_bad_points, self.bad_point = int(info.n_bad_points), int(info.bad_point)
        self.min_pivot_rel, self.kernel_us = float(info.min_pivot_rel), float(info.kernel_us)

    @property
    def ok(self):
        return self.status == 0

    def __repr__(self):
        return (f"Covariance(status={self.STATUS.get(self.status, self.status)!r}, sigma2={self.sigma2:.6g}, dof={self.dof}, "
                f"gauge={self.gauge}, n_free={self.n_free}, n_held={self.n_held}, min_pivot_rel={self.min_pivot_rel:.3g}, "
                f"bad_param={self.bad_param}, n_bad_points={self.n_bad_points})")


class Triangulation:
    """What `Backend.triangulate` returns (include/sfmba.h: sfmba_triangulate).  ``points`` (P, 3): the new point where
    ``status`` is 0, else the point of ``x``; ``status`` (P) one of the ``Triangulation.OK .. HIGH_ERROR`` codes, -1 for a
    point that was not selected; ``views``, ``iters`` (P, int32); ``rms_err`` (pixels) and ``angle_deg`` (P), NaN where
    the point did not get that far; ``n_ok`` the number of status-0 points."""

    NOT_SELECTED, OK, FEW_VIEWS, AT_INFINITY, BEHIND, LOW_ANGLE, HIGH_ERROR = -1, 0, 1, 2, 3, 4, 5

    def __init__(self, points, status, views, iters, rms_err, angle_deg, n_ok):
        self.points, self.status, self.views, self.iters = points, status, views, iters
        self.rms_err, self.angle_deg, self.n_ok = rms_err, angle_deg, int(n_ok)

    @property
    def ok(self):
        """Boolean mask of the points that came back with a new position."""
        return self.status == self.OK

    def __repr__(self):
        return f"Triangulation(n_points={len(self.status)}, n_ok={self.n_ok})"


class RobustTriangulation(Triangulation):
    """What `Backend.triangulate_ransac` returns (include/sfmba.h: sfmba_triangulate_ransac): the fields of
    :class:`Triangulation` -- ``points`` the refined point where ``status`` is 0, ``views`` the used observations,
    ``iters``, ``rms_err`` and ``angle_deg`` those of the refinement over the inliers -- and ``hyp`` (P, 3) the best
    hypothesis' point, unrefined; ``inlier_mask`` (N, bool) in the caller's observation order; ``inliers``, ``best`` (the
    winning hypothesis) (P, int32); ``hyp_inliers`` (P, H) the count of every hypothesis, or None when not asked for;
    ``kernel_us`` (``profile=1``, else 0).  ``status`` may also be ``NO_CONSENSUS``."""

    NO_CONSENSUS = 6

    def __init__(self, points, status, views, iters, rms_err, angle_deg, n_ok, hyp, inlier_mask, inliers, best,
                 hyp_inliers, kernel_us=0.0):
        super().__init__(points, status, views, iters, rms_err, angle_deg, n_ok)
        self.hyp, self.inlier_mask, self.inliers, self.best = hyp, inlier_mask, inliers, best
        self.hyp_inliers, self.kernel_us = hyp_inliers, float(kernel_us)

    def __repr__(self):
        return f"RobustTriangulation(n_points={len(self.status)}, n_ok={self.n_ok})"


class Resection:
    """What `Backend.resect` returns (include/sfmba.h: sfmba_resect).  ``cameras`` (C, 6): the new pose (rotation vector,
    centre -- the bundle-adjustment model's parameters) where ``status`` is 0, else the camera of ``x``; ``status`` (C)
    one of the ``Resection.OK .. HIGH_ERROR`` codes, -1 for a camera that was not selected; ``views``, ``iters`` (C,
    int32); ``rms_err`` (pixels), NaN where the camera did not get that far; ``n_ok`` the number of status-0 cameras."""

    NOT_SELECTED, OK, FEW_VIEWS, DEGENERATE, BEHIND, HIGH_ERROR = -1, 0, 1, 2, 3, 4

    def __init__(self, cameras, status, views, iters, rms_err, n_ok):
        self.cameras, self.status, self.views, self.iters = cameras, status, views, iters
        self.rms_err, self.n_ok = rms_err, int(n_ok)

    @property
    def ok(self):
        """Boolean mask of the cameras that came back with a new pose."""
        return self.status == self.OK

    def __repr__(self):
        return f"Resection(n_cameras={len(self.status)}, n_ok={self.n_ok})"


@dataclasses.dataclass
class RobustResection:
    """What `Backend.resect_ransac` returns (include/sfmba.h: sfmba_resect_ransac).  ``cameras`` (C, 6): the refined pose
    (rotation vector, centre) where ``status`` is 0, else the camera of ``x``; ``hyp`` (C, 6): the best hypothesis' pose,
    unrefined; ``inlier_mask`` (N, bool) in the caller's observation order; ``status`` (C) one of the ``NOT_SELECTED ..
    HIGH_ERROR`` codes; ``views``, ``inliers``, ``best`` (the winning hypothesis), ``best_sol`` (its solution), ``iters``
    (C, int32); ``success`` (C, bool): inliers / views >= confidence; ``rms_err`` (C) over the inliers, NaN where the
    camera did not get that far; ``hyp_inliers`` (C, H) the count of every hypothesis, or None when not asked for;
    ``n_ok``; ``kernel_us`` (``profile=1``, else 0)."""

    NOT_SELECTED, OK, FEW_VIEWS, DEGENERATE, BEHIND, HIGH_ERROR = -1, 0, 1, 2, 3, 4

    cameras: np.ndarray
    hyp: np.ndarray
    inlier_mask: np.ndarray
    status: np.ndarray
    views: np.ndarray
    inliers: np.ndarray
    best: np.ndarray
    best_sol: np.ndarray
    success: np.ndarray
    iters: np.ndarray
    rms_err: np.ndarray
    hyp_inliers: object
    n_ok: int
    kernel_us: float

    @property
    def ok(self):
        """Boolean mask of the cameras that came back with a new pose."""
        return self.status == self.OK

    def __repr__(self):
        return f"RobustResection(n_cameras={len(self.status)}, n_ok={self.n_ok})"
