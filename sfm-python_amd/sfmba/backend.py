"""Handle wrapper around the C-ABI: owns one sfmba_handle (one GPU, one problem at a time)."""
from __future__ import annotations

import ctypes as C
import dataclasses

import weakref

import numpy as np

from . import _capi


class FundamentalEstimate:
    """What `Backend.fundamental_ransac` returns (include/sfmba.h: sfmba_fundamental_ransac), per edge of the batch:
    ``F`` and ``F_refit`` (E, 3, 3), unit Frobenius norm, largest entry positive (``F_refit`` equals ``F`` unless
    ``refit=1``); ``inliers``, ``best`` (the winning hypothesis), ``status`` (one of ``OK, FEW_PAIRS, DEGENERATE``) as
    int32 (E), ``success`` (E, bool): inliers / used pairs >= confidence; ``inlier_mask`` (M, bool) over the stored pairs;
    ``hyp_inliers`` (E, H) the count of every hypothesis, or None when not asked for; ``n_ok``; ``kernel_us``
    (``profile=1``, else 0)."""

    OK, FEW_PAIRS, DEGENERATE = 0, 1, 2

    def __init__(self, F, F_refit, inlier_mask, inliers, best, success, status, hyp_inliers, n_ok, kernel_us, edge_ptr):
        self.F, self.F_refit, self.inlier_mask = F, F_refit, inlier_mask
        self.inliers, self.best, self.success, self.status = inliers, best, success, status
        self.hyp_inliers, self.n_ok, self.kernel_us, self.edge_ptr = hyp_inliers, int(n_ok), float(kernel_us), edge_ptr

    @property
    def ok(self):
        return self.status == self.OK

    def __repr__(self):
        return f"FundamentalEstimate(n_edges={len(self.status)}, n_ok={self.n_ok})"


class HomographyEstimate:
    """What `Backend.homography_ransac` returns (include/sfmba.h: sfmba_homography_ransac), per edge of the batch:
    ``H`` and ``H_refit`` (E, 3, 3), ``x2 ~ H x1``, unit Frobenius norm, largest entry positive (``H_refit`` equals ``H``
    unless ``refit=1``); ``inliers``, ``refit_inliers``, ``best`` (the winning hypothesis), ``status`` (one of ``OK,
    FEW_PAIRS, DEGENERATE``) as int32 (E), ``success`` (E, bool): inliers / used pairs >= confidence; ``inlier_mask`` (of
    ``H``) and ``refit_mask`` (of ``H_refit``) (M, bool) over the stored pairs; ``hyp_inliers`` (E, H) the count of every
    hypothesis, or None when not asked for; ``n_ok``; ``kernel_us`` (``profile=1``, else 0)."""

    OK, FEW_PAIRS, DEGENERATE = 0, 1, 2

    def __init__(self, H, H_refit, inlier_mask, refit_mask, inliers, refit_inliers, best, success, status, hyp_inliers, n_ok,
                 kernel_us, edge_ptr):
        self.H, self.H_refit, self.inlier_mask, self.refit_mask = H, H_refit, inlier_mask, refit_mask
        self.inliers, self.refit_inliers, self.best, self.success, self.status = inliers, refit_inliers, best, success, status
        self.hyp_inliers, self.n_ok, self.kernel_us, self.edge_ptr = hyp_inliers, int(n_ok), float(kernel_us), edge_ptr

    @property
    def ok(self):
        return self.status == self.OK

    def __repr__(self):
        return f"HomographyEstimate(n_edges={len(self.status)}, n_ok={self.n_ok})"


class SimilarityEstimate:
    """What `Backend.similarity_ransac` returns (include/sfmba.h: sfmba_similarity_ransac), per set of the batch:
    ``dst ~ scale R src + t`` with ``scale`` (E), ``R`` (E, 3, 3), ``t`` (E, 3) of the best hypothesis and ``scale_refit``,
    ``R_refit``, ``t_refit`` of the estimate over all its inliers (copies unless ``refit=1``); ``inliers``,
    ``refit_inliers``, ``best`` (the winning hypothesis), ``status`` (one of ``OK, FEW_PAIRS, DEGENERATE``) as int32 (E),
    ``success`` (E, bool): inliers / used pairs >= confidence; ``inlier_mask`` (of the best hypothesis) and ``refit_mask``
    (of the refit) (M, bool) over the stored pairs; ``hyp_inliers`` (E, H) the count of every hypothesis, or None when not
    asked for; ``n_ok``; ``kernel_us`` (``profile=1``, else 0); ``set_ptr``.  A status OK says only that three or more
    pairs agree: how many inliers are enough is the caller's decision."""

    OK, FEW_PAIRS, DEGENERATE = 0, 1, 2

    def __init__(self, sim, sim_refit, inlier_mask, refit_mask, inliers, refit_inliers, best, success, status, hyp_inliers, n_ok,
                 kernel_us, set_ptr):
        self.scale, self.R, self.t = sim[:, 0].copy(), sim[:, 1:10].reshape(-1, 3, 3).copy(), sim[:, 10:13].copy()
        self.scale_refit, self.R_refit, self.t_refit = (sim_refit[:, 0].copy(), sim_refit[:, 1:10].reshape(-1, 3, 3).copy(),
                                                        sim_refit[:, 10:13].copy())
        self.inlier_mask, self.refit_mask = inlier_mask, refit_mask
        self.inliers, self.refit_inliers, self.best, self.success, self.status = inliers, refit_inliers, best, success, status
        self.hyp_inliers, self.n_ok, self.kernel_us, self.set_ptr = hyp_inliers, int(n_ok), float(kernel_us), set_ptr

    @property
    def ok(self):
        return self.status == self.OK

    def __repr__(self):
        return f"SimilarityEstimate(n_sets={len(self.status)}, n_ok={self.n_ok})"


class EssentialEstimate:
    """What `Backend.essential_ransac` returns (include/sfmba.h: sfmba_essential_ransac), per edge of the batch: ``E``
    (n_edges, 3, 3), unit Frobenius norm, largest entry positive (compare up to sign); ``inliers``, ``best`` (the winning
    hypothesis), ``best_root`` (its candidate, by ascending z), ``status`` (one of ``OK, FEW_PAIRS, DEGENERATE``) as int32
    (n_edges), ``success`` (n_edges, bool): inliers / used pairs >= confidence; ``inlier_mask`` (M, bool) over the stored
    pairs; ``hyp_inliers`` and ``hyp_roots`` (n_edges, H) the count and the number of real roots of every hypothesis, or
    None when not asked for; ``n_ok``; ``kernel_us`` (``profile=1``, else 0)."""

    OK, FEW_PAIRS, DEGENERATE = 0, 1, 2

    def __init__(self, E, inlier_mask, inliers, best, best_root, success, status, hyp_inliers, hyp_roots, n_ok, kernel_us, edge_ptr):
        self.E, self.inlier_mask = E, inlier_mask
        self.inliers, self.best, self.best_root, self.success, self.status = inliers, best, best_root, success, status
        self.hyp_inliers, self.hyp_roots = hyp_inliers, hyp_roots
        self.n_ok, self.kernel_us, self.edge_ptr = int(n_ok), float(kernel_us), edge_ptr

    @property
    def ok(self):
        return self.status == self.OK

    def __repr__(self):
        return f"EssentialEstimate(n_edges={len(self.status)}, n_ok={self.n_ok})"


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


def check_descriptors(descs):
    """A list of (n_i, D) descriptor arrays, checked -> (desc (N, D) uint8 or float32, img_ptr (n + 1) int64).  All uint8:
    kept as uint8; otherwise everything is converted to float32."""
    if isinstance(descs, np.ndarray) and descs.ndim == 2:
        raise ValueError("descs must be a list of (n_i, D) arrays, one per image, not one array")
    arrs = [np.asarray(d) for d in descs]
    for k, a in enumerate(arrs):
        if a.ndim != 2:
            raise ValueError(f"descriptors of image {k} must be (n, D), got shape {a.shape}")
        if not (np.issubdtype(a.dtype, np.number) or a.dtype == np.bool_) or np.issubdtype(a.dtype, np.complexfloating):
            raise ValueError(f"descriptors of image {k} have dtype {a.dtype}")
    if not arrs:
        return np.empty((0, 1), dtype=np.uint8), np.zeros(1, dtype=np.int64)
    D = arrs[0].shape[1]
    if any(a.shape[1] != D for a in arrs):
        raise ValueError(f"all images must have the same descriptor length, got {sorted({a.shape[1] for a in arrs})}")
    if not 1 <= D <= 512:
        raise ValueError(f"descriptor length must be 1..512, got {D}")
    dt = np.uint8 if all(a.dtype == np.uint8 for a in arrs) else np.float32
    desc = np.ascontiguousarray(np.concatenate([a.astype(dt, copy=False) for a in arrs], axis=0))
    ptr = np.concatenate([[0], np.cumsum([len(a) for a in arrs])]).astype(np.int64)
    return desc, ptr


def check_match_edges(edges, n_images):
    """(E, 2) int32 of (query image, train image), checked against the number of images; None: all pairs u > v in the
    order of the reference's ``product(nodes, repeat=2)`` (sfm.py:90)."""
    if edges is None:
        edges = [(u, v) for u in range(n_images) for v in range(n_images) if u > v]
    e = np.asarray(edges)
    if e.size == 0:
        return np.empty((0, 2), dtype=np.int32)
    if e.ndim == 1 and e.shape[0] == 2:
        e = e[None]
    if e.ndim != 2 or e.shape[1] != 2:
        raise ValueError(f"edges must be (E, 2), got {e.shape}")
    if not np.issubdtype(e.dtype, np.integer):
        raise ValueError(f"edges must be integers, got {e.dtype}")
    if e.min() < 0 or e.max() >= n_images:
        raise ValueError(f"edges name image {int(e.max() if e.max() >= n_images else e.min())}, the set has {n_images}")
    return np.ascontiguousarray(e, dtype=np.int32)


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


def check_track_inputs(img_ptr, edges, pair_ptr, pairs, pair_use=None, min_length=2, max_length=0, conflicts=0, profile=0):
    """The arguments of `Backend.build_tracks`, checked as sfmba_build_tracks checks them -> (img_ptr int64, edges (E, 2)
    int32, pair_ptr int64, pairs (M, 2) int32, pair_use uint8 or None, options dict).  Raises ValueError."""
    def ascending(a, name):
        a = np.asarray(a)
        if a.ndim != 1 or a.shape[0] < 1 or not (np.issubdtype(a.dtype, np.integer) or a.dtype == np.bool_):
            raise ValueError(f"{name} must be a non-empty 1-D integer array")
        a = np.ascontiguousarray(a, dtype=np.int64)
        if a[0] != 0 or np.any(np.diff(a) < 0):
            raise ValueError(f"{name} must ascend from 0")
        return a

    def int_pairs(a, name):
        a = np.asarray(a)
        if a.size == 0:
            return np.empty((0, 2), dtype=np.int32)
        if a.ndim != 2 or a.shape[1] != 2:
            raise ValueError(f"{name} must be (n, 2), got {a.shape}")
        if not np.issubdtype(a.dtype, np.integer):
            raise ValueError(f"{name} must be integers, got {a.dtype}")
        if a.min() < -2**31 or a.max() >= 2**31:
            raise ValueError(f"{name} does not fit int32")
        return np.ascontiguousarray(a, dtype=np.int32)

    for name, v in (("min_length", min_length), ("max_length", max_length), ("conflicts", conflicts)):
        if int(v) != v:
            raise ValueError(f"{name} must be an integer, got {v!r}")
    min_length, max_length, conflicts = int(min_length), int(max_length), int(conflicts)
    if min_length < 1:
        raise ValueError(f"min_length must be at least 1, got {min_length}")
    if max_length < 0 or (max_length and max_length < min_length):
        raise ValueError(f"max_length {max_length} is below min_length {min_length} (0 = no limit)")
    if conflicts not in (0, 1):
        raise ValueError(f"conflicts must be 0 (drop) or 1 (keep), got {conflicts}")
    img_ptr, pair_ptr = ascending(img_ptr, "img_ptr"), ascending(pair_ptr, "pair_ptr")
    n_images, N = len(img_ptr) - 1, int(img_ptr[-1])
    if N >= 2**31:
        raise ValueError(f"{N} features, the limit is 2^31 - 1")
    edges, pairs = int_pairs(edges, "edges"), int_pairs(pairs, "pairs")
    if len(edges) != len(pair_ptr) - 1:
        raise ValueError(f"{len(edges)} edges, pair_ptr is for {len(pair_ptr) - 1}")
    if len(pairs) != pair_ptr[-1]:
        raise ValueError(f"{len(pairs)} pairs, pair_ptr ends at {int(pair_ptr[-1])}")
    if len(edges):
        if edges.min() < 0 or edges.max() >= n_images:
            raise ValueError(f"edges name image {int(edges.max() if edges.max() >= n_images else edges.min())}, there are {n_images}")
        same = np.flatnonzero(edges[:, 0] == edges[:, 1])
        if len(same):
            raise ValueError(f"edge {int(same[0])} joins image {int(edges[same[0], 0])} to itself")
    if len(pairs):
        rows = np.diff(img_ptr).astype(np.uint32)
        limit = np.repeat(rows[edges], np.diff(pair_ptr), axis=0)            # (M, 2): rows of u, rows of v
        bad = pairs.view(np.uint32) >= limit                                 # (unsigned: a negative row is a huge one)
        if bad.any():
            raise ValueError(f"pair {int(np.flatnonzero(bad.any(axis=1))[0])} names a row outside its image")
    pair_use = _mask(pair_use, len(pairs), "pair_use")
    return img_ptr, edges, pair_ptr, pairs, pair_use, dict(min_length=min_length, max_length=max_length,
                                                           conflicts=conflicts, profile=int(bool(profile)))


def check_plan_inputs(n_images=None, n_tracks=None, cam_mask=None, trk_mask=None, min_views=2, keypoints=None, img_ptr=None):
    """The arguments of `Backend.plan_views`, `Backend.assemble_problem` and `Backend.set_keypoints`, checked as the C side
    checks them (csrc/plan_inputs.hpp) -> ``(cam_mask uint8, trk_mask uint8, min_views, pts (N, 2) float64, kp_ptr int64)``.
    ``n_images`` / ``n_tracks``: the sizes of the last build, None = no masks to check; ``keypoints``: a list of (n_i, 2)
    pixel arrays, one per image, None = none to check; ``img_ptr``: the tracks' img_ptr the keypoints must agree with.
    Raises ValueError."""
    cam = trk = pts = kp_ptr = None
    if int(min_views) != min_views:
        raise ValueError(f"min_views must be an integer, got {min_views!r}")
    min_views = int(min_views)
    if min_views < 1:
        raise ValueError(f"min_views must be at least 1, got {min_views}")
    if n_images is not None:
        for name, a, n in (("image", cam_mask, int(n_images)), ("track", trk_mask, int(n_tracks))):
            if a is None:
                raise ValueError(f"the {name} mask is missing")
            if np.asarray(a).ndim != 1:
                raise ValueError(f"the {name} mask must be 1-D, got shape {np.asarray(a).shape}")
        cam, trk = _mask(cam_mask, int(n_images), "the image mask"), _mask(trk_mask, int(n_tracks), "the track mask")
    if keypoints is not None:
        if isinstance(keypoints, np.ndarray) and keypoints.ndim == 2:
            raise ValueError("keypoints must be a list of (n_i, 2) arrays, one per image, not one array")
        arrs = [np.asarray(p, dtype=np.float64) for p in keypoints]
        for k, a in enumerate(arrs):
            if a.ndim != 2 or a.shape[1] != 2:
                if a.size:
                    raise ValueError(f"pixels of image {k} must be (n, 2), got shape {a.shape}")
                arrs[k] = a.reshape(0, 2)
            if not np.all(np.isfinite(a)):
                raise ValueError(f"a pixel of image {k} is not finite")
        kp_ptr = np.concatenate([[0], np.cumsum([len(a) for a in arrs])]).astype(np.int64)
        if kp_ptr[-1] >= 2**31:
            raise ValueError(f"{int(kp_ptr[-1])} features, the limit is 2^31 - 1")
        if img_ptr is not None:
            img_ptr = np.asarray(img_ptr, dtype=np.int64).ravel()
            if img_ptr.shape[0] < 1 or img_ptr[0] != 0 or np.any(np.diff(img_ptr) < 0):
                raise ValueError("img_ptr must ascend from 0")
            if not np.array_equal(img_ptr, kp_ptr):
                raise ValueError("the keypoints' row counts differ from the tracks' img_ptr")
        pts = np.ascontiguousarray(np.concatenate(arrs, axis=0) if arrs else np.empty((0, 2)))
    return cam, trk, min_views, pts, kp_ptr


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


def check_match_options(ratio=0.5, form=0, profile=0):
    ratio = float(ratio)
    if not ratio > 0.0:
        raise ValueError(f"ratio must be positive, got {ratio}")
    if form not in (0, 1, 2):
        raise ValueError(f"form must be 0 (auto), 1 (A) or 2 (B), got {form!r}")
    return ratio, int(form), int(bool(profile))


def _edge_batch(pts1, pts2, edge_ptr, pair_use, dim=2, names=("pts1", "pts2", "edge_ptr")):
    """The arrays of a batch of edges, checked: pts1, pts2 (M, dim) float64, edge_ptr (E + 1) int64 ascending from 0 to M
    (None: one edge), the mask (M) uint8 or None.  (dim = 3 and the names of `similarity_ransac`: a batch of sets.)"""
    pts1, pts2 = _f64(pts1), _f64(pts2)
    if pts1.ndim != 2 or pts1.shape[1] != dim or pts2.shape != pts1.shape:
        raise ValueError(f"{names[0]} and {names[1]} must both be (M, {dim}), got {pts1.shape} and {pts2.shape}")
    M = pts1.shape[0]
    if edge_ptr is None:
        edge_ptr = np.array([0, M], dtype=np.int64)
    edge_ptr = np.ascontiguousarray(edge_ptr, dtype=np.int64).ravel()
    if edge_ptr.shape[0] < 1 or edge_ptr[0] != 0 or edge_ptr[-1] != M or np.any(np.diff(edge_ptr) < 0):
        raise ValueError(f"{names[2]} must ascend from 0 to the number of pairs")
    return pts1, pts2, edge_ptr, _mask(pair_use, M, "pair_use")


def check_similarity_inputs(src, dst, set_ptr=None, pair_use=None, samples=None, **options):
    """The arguments of `Backend.similarity_ransac`, checked without a device -> ``(src, dst, set_ptr, pair_use, samples,
    options)``: ``src``, ``dst`` (M, 3) float64; ``set_ptr`` (E + 1) int64 ascending from 0 to M (None: one set);
    ``pair_use`` (M) uint8 or None; ``samples`` (E, H, 3) int32 or None ((H, 3) stands for one set); ``options`` a
    `_capi.RansacOptions` holding the library's defaults (threshold 1.0, confidence 0.99, seed 0, max_iters 1000 or the
    samples' H, refit 0, profile 0) overridden by the keywords.  Raises ``ValueError`` for a wrong shape, a
    non-ascending ``set_ptr``, a NaN option, ``max_iters < 1`` or samples that disagree with it, ``TypeError`` for an
    unknown keyword.  (Whether a sample position lies inside its set depends on the mask: the library checks it.)"""
    src, dst, set_ptr, use = _edge_batch(src, dst, set_ptr, pair_use, dim=3, names=("src", "dst", "set_ptr"))
    opt = _capi.RansacOptions(threshold=1.0, confidence=0.99, seed=0, max_iters=1000, refit=0, profile=0)
    samples = _ransac_prologue(opt, options, samples, set_ptr.shape[0] - 1, 3, "n_sets", "set", "similarity RANSAC")
    if np.isnan(opt.threshold) or np.isnan(opt.confidence):
        raise ValueError("an option of the similarity RANSAC is NaN")
    return src, dst, set_ptr, use, samples, opt


def _ransac_prologue(opt, options, samples, batch, S, batch_name, item, what, then_flush=None):
    """The keyword options and the caller's sample sets of a RANSAC call, checked: the options into ``opt`` (a ctypes
    structure holding the defaults; ``what`` names the call in an error text) -> the samples as (batch, H, S) int32,
    C-contiguous, None staying None.  ``seed`` must fit 64 unsigned bits; with samples given ``max_iters`` defaults to
    their H and must equal it.  The samples are converted to int32 and (H, S) stands for a batch of one, checked after the
    seed; with ``then_flush`` (`Backend.homography_ransac`) they must come as three axes of an integer type and are
    checked first, and ``then_flush()`` runs before any other check."""
    strict = then_flush is not None

    def shaped(s):
        if s is None:
            return None
        if strict:
            s = np.asarray(s)
            right, kind, got = s.dtype.kind in "iu" and s.ndim == 3, " int32", f"{s.dtype} {s.shape}"
        else:
            s = np.ascontiguousarray(s, dtype=np.int32)
            s = s[None] if s.ndim == 2 else s
            right, kind, got = s.ndim == 3, "", f"{s.shape}"
        if not right or s.shape[0] != batch or s.shape[2] != S or s.shape[1] < 1:
            raise ValueError(f"samples must be ({batch_name}, H, {S}){kind} with {batch_name} = {batch}, got {got}")
        return np.ascontiguousarray(s, dtype=np.int32)

    if strict:
        samples = shaped(samples)
        then_flush()
    options = dict(options)
    if "seed" in options:
        seed = int(options.pop("seed"))
        if not 0 <= seed < 2 ** 64:
            raise ValueError("seed must fit 64 unsigned bits")
        opt.seed = seed
    if not strict:
        samples = shaped(samples)
    if samples is not None:
        options.setdefault("max_iters", samples.shape[1])
    _fill_options(opt, options, what)
    if opt.max_iters < 1:
        raise ValueError("max_iters must be at least 1")
    if samples is not None and samples.shape[1] != opt.max_iters:
        raise ValueError(f"samples holds {samples.shape[1]} hypotheses per {item}, max_iters is {opt.max_iters}")
    return samples


def check_essential_args(K, options):
    """``K`` of `Backend.essential_ransac` as (3, 3) float64, finite and invertible, and its ``options`` without a refit:
    there is no refit of an essential matrix (include/sfmba.h: sfmba_essential_ransac, "Not done here")."""
    K = np.ascontiguousarray(K, dtype=np.float64)
    if K.shape != (3, 3):
        raise ValueError(f"K must be (3, 3), got {K.shape}")
    if not np.all(np.isfinite(K)):
        raise ValueError("K must be finite")
    with np.errstate(all="ignore"):
        invertible = float(np.linalg.det(K)) != 0.0 and bool(np.all(np.isfinite(np.linalg.inv(K))))
    if not invertible:
        raise ValueError("K must be invertible")
    if int(options.get("refit", 0)) != 0:
        raise ValueError("refit must be 0: an essential matrix has no refit")
    return K


def _opt_ptr(a):
    return _capi.ptr(a) if a is not None else None


class BackendError(RuntimeError):
    pass


def _f64(a, shape=None, name="array"):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None and a.shape != shape:
        raise ValueError(f"{name} has shape {a.shape}, expected {shape}")
    return a


def _mask(a, n, name):
    """A boolean mask of n entries as contiguous uint8 (None stays None: every entry)."""
    if a is None:
        return None
    a = np.ascontiguousarray(np.asarray(a).ravel() != 0, dtype=np.uint8)
    if a.shape[0] != n:
        raise ValueError(f"{name} has {a.shape[0]} entries, expected {n}")
    return a


def _fill_options(opt, options, what):
    """Keyword options into the fields of the ctypes structure `opt`; `what` names the call in the error text."""
    names = {f[0]: f[1] for f in type(opt)._fields_}
    for key, value in options.items():
        if key not in names:
            raise TypeError(f"unknown {what} option {key!r} (known: {sorted(names)})")
        setattr(opt, key, int(value) if names[key] is C.c_int32 else float(value))


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

    def fundamental_ransac(self, pts1, pts2, edge_ptr=None, pair_use=None, samples=None, want_hyp=False, **options):
        """F by RANSAC for every edge of a batch of matched pixel pairs, the reference's
        ``estimate_fundamental_matrix_ransac`` (include/sfmba.h: sfmba_fundamental_ransac).  ``pts1``, ``pts2`` (M, 2);
        ``edge_ptr`` (E + 1) the edges' runs, None = one edge; ``pair_use`` (M) boolean, None = all; ``samples``
        (E, H, 8) int32 positions among an edge's used pairs, None = drawn on the device from ``seed``.  ``options``:
        fields of ``sfmba_ransac_options`` (threshold, confidence, seed, max_iters, refit, profile); with ``samples``
        given, ``max_iters`` defaults to its H.  ``want_hyp``: also return the count of every hypothesis.  Needs no
        problem.  -> :class:`FundamentalEstimate`."""
        self._flush_pending()
        pts1, pts2, edge_ptr, use = _edge_batch(pts1, pts2, edge_ptr, pair_use)
        E, M = edge_ptr.shape[0] - 1, pts1.shape[0]
        opt = _capi.RansacOptions()
        self._lib.sfmba_default_ransac_options(C.byref(opt))
        samples = _ransac_prologue(opt, options, samples, E, 8, "n_edges", "edge", "RANSAC")
        H = int(opt.max_iters)
        F, Fr = np.empty((E, 3, 3)), np.empty((E, 3, 3))
        mask = np.empty(M, dtype=np.uint8)
        inl, best, status = (np.empty(E, dtype=np.int32) for _ in range(3))
        success = np.empty(E, dtype=np.uint8)
        hyp = np.empty((E, H), dtype=np.int32) if want_hyp else None
        n_ok, us = C.c_int64(), C.c_double()
        self._check(self._lib.sfmba_fundamental_ransac(
            self._h, E, _capi.ptr(edge_ptr), _capi.ptr(pts1), _capi.ptr(pts2), _opt_ptr(use), _opt_ptr(samples), C.byref(opt),
            _capi.ptr(F), _capi.ptr(Fr), _capi.ptr(mask), _capi.ptr(inl), _capi.ptr(best), _capi.ptr(success),
            _capi.ptr(status), _opt_ptr(hyp), C.byref(n_ok), C.byref(us)))
        return FundamentalEstimate(F, Fr, mask.view(np.bool_), inl, best, success.view(np.bool_), status, hyp, n_ok.value,
                                   us.value, edge_ptr)

    def homography_ransac(self, pts1, pts2, edge_ptr=None, pair_use=None, samples=None, want_hyp=False, **options):
        """A homography ``x2 ~ H x1`` by RANSAC for every edge of a batch of matched pixel pairs (include/sfmba.h:
        sfmba_homography_ransac), the sibling of :meth:`fundamental_ransac`: the same batch arguments and the same
        ``options`` (fields of ``sfmba_ransac_options``); ``samples`` (E, H, 4) int32 positions among an edge's used
        pairs, None = drawn on the device from ``seed``; with ``samples`` given, ``max_iters`` defaults to its H.
        ``want_hyp``: also return the count of every hypothesis.  Needs no problem.  -> :class:`HomographyEstimate`."""
        pts1, pts2, edge_ptr, use = _edge_batch(pts1, pts2, edge_ptr, pair_use)
        E, M = edge_ptr.shape[0] - 1, pts1.shape[0]
        opt = _capi.RansacOptions()
        self._lib.sfmba_default_ransac_options(C.byref(opt))
        samples = _ransac_prologue(opt, options, samples, E, 4, "n_edges", "edge", "RANSAC", then_flush=self._flush_pending)
        H = int(opt.max_iters)
        Hm, Hr = np.empty((E, 3, 3)), np.empty((E, 3, 3))
        mask, rmask = np.empty(M, dtype=np.uint8), np.empty(M, dtype=np.uint8)
        inl, rinl, best, status = (np.empty(E, dtype=np.int32) for _ in range(4))
        success = np.empty(E, dtype=np.uint8)
        hyp = np.empty((E, H), dtype=np.int32) if want_hyp else None
        n_ok, us = C.c_int64(), C.c_double()
        self._check(self._lib.sfmba_homography_ransac(
            self._h, E, _capi.ptr(edge_ptr), _capi.ptr(pts1), _capi.ptr(pts2), _opt_ptr(use), _opt_ptr(samples), C.byref(opt),
            _capi.ptr(Hm), _capi.ptr(Hr), _capi.ptr(mask), _capi.ptr(rmask), _capi.ptr(inl), _capi.ptr(rinl), _capi.ptr(best),
            _capi.ptr(success), _capi.ptr(status), _opt_ptr(hyp), C.byref(n_ok), C.byref(us)))
        return HomographyEstimate(Hm, Hr, mask.view(np.bool_), rmask.view(np.bool_), inl, rinl, best, success.view(np.bool_),
                                  status, hyp, n_ok.value, us.value, edge_ptr)

    def similarity_ransac(self, src, dst, set_ptr=None, pair_use=None, samples=None, want_hyp=False, **options):
        """A similarity ``dst ~ s R src + t`` by RANSAC for every set of a batch of 3-D point pairs (include/sfmba.h:
        sfmba_similarity_ransac), the fifth model of the family: ``src``, ``dst`` (M, 3); ``set_ptr`` (E + 1) the sets'
        runs, None = one set; ``pair_use`` (M) boolean, None = all; ``samples`` (E, H, 3) int32 positions among a set's used
        pairs, None = drawn on the device from ``seed``; ``options``: fields of ``sfmba_ransac_options`` -- ``threshold``
        is a distance in the units of ``dst``, so pass one --; with ``samples`` given, ``max_iters`` defaults to its H.
        ``want_hyp``: also return the count of every hypothesis.  Needs no problem.  -> :class:`SimilarityEstimate`."""
        src, dst, set_ptr, use, samples, opt = check_similarity_inputs(src, dst, set_ptr, pair_use, samples, **options)
        self._flush_pending()
        E, M, H = set_ptr.shape[0] - 1, src.shape[0], int(opt.max_iters)
        sim, simr = np.empty((E, 13)), np.empty((E, 13))
        mask, rmask = np.empty(M, dtype=np.uint8), np.empty(M, dtype=np.uint8)
        inl, rinl, best, status = (np.empty(E, dtype=np.int32) for _ in range(4))
        success = np.empty(E, dtype=np.uint8)
        hyp = np.empty((E, H), dtype=np.int32) if want_hyp else None
        n_ok, us = C.c_int64(), C.c_double()
        self._check(self._lib.sfmba_similarity_ransac(
            self._h, E, _capi.ptr(set_ptr), _capi.ptr(src), _capi.ptr(dst), _opt_ptr(use), _opt_ptr(samples), C.byref(opt),
            _capi.ptr(sim), _capi.ptr(simr), _capi.ptr(mask), _capi.ptr(rmask), _capi.ptr(inl), _capi.ptr(rinl), _capi.ptr(best),
            _capi.ptr(success), _capi.ptr(status), _opt_ptr(hyp), C.byref(n_ok), C.byref(us)))
        return SimilarityEstimate(sim, simr, mask.view(np.bool_), rmask.view(np.bool_), inl, rinl, best, success.view(np.bool_),
                                  status, hyp, n_ok.value, us.value, set_ptr)

    def essential_ransac(self, pts1, pts2, K, edge_ptr=None, pair_use=None, samples=None, want_hyp=False, **options):
        """The essential matrix by five-point RANSAC for every edge of a batch of matched pixel pairs (include/sfmba.h:
        sfmba_essential_ransac), the calibrated sibling of :meth:`fundamental_ransac`: the same batch arguments and the
        same ``options`` (fields of ``sfmba_ransac_options``; ``refit`` must stay 0); ``K`` (3, 3) the one camera matrix of
        both images; ``samples`` (E, H, 5) int32 positions among an edge's used pairs, None = drawn on the device from
        ``seed``; with ``samples`` given, ``max_iters`` defaults to its H.  ``want_hyp``: also return the count and the
        number of real roots of every hypothesis.  Needs no problem.  -> :class:`EssentialEstimate`."""
        pts1, pts2, edge_ptr, use = _edge_batch(pts1, pts2, edge_ptr, pair_use)
        K = check_essential_args(K, options)
        E, M = edge_ptr.shape[0] - 1, pts1.shape[0]
        opt = _capi.RansacOptions()
        self._lib.sfmba_default_ransac_options(C.byref(opt))
        samples = _ransac_prologue(opt, options, samples, E, 5, "n_edges", "edge", "RANSAC", then_flush=self._flush_pending)
        H = int(opt.max_iters)
        Em = np.empty((E, 3, 3))
        mask = np.empty(M, dtype=np.uint8)
        inl, best, root, status = (np.empty(E, dtype=np.int32) for _ in range(4))
        success = np.empty(E, dtype=np.uint8)
        hyp = np.empty((E, H), dtype=np.int32) if want_hyp else None
        hyp_roots = np.empty((E, H), dtype=np.int32) if want_hyp else None
        n_ok, us = C.c_int64(), C.c_double()
        self._check(self._lib.sfmba_essential_ransac(
            self._h, E, _capi.ptr(edge_ptr), _capi.ptr(pts1), _capi.ptr(pts2), _opt_ptr(use), _opt_ptr(samples), _capi.ptr(K),
            C.byref(opt), _capi.ptr(Em), _capi.ptr(mask), _capi.ptr(inl), _capi.ptr(best), _capi.ptr(root), _capi.ptr(success),
            _capi.ptr(status), _opt_ptr(hyp), _opt_ptr(hyp_roots), C.byref(n_ok), C.byref(us)))
        return EssentialEstimate(Em, mask.view(np.bool_), inl, best, root, success.view(np.bool_), status, hyp, hyp_roots,
                                 n_ok.value, us.value, edge_ptr)

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
