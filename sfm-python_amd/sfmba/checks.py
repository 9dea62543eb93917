"""Device-free argument checks and conversions of the `Backend` calls: nothing here needs the library or a GPU."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi


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


def _ransac_prologue(opt, options, samples, batch, S, batch_name, item, what, strict=False):
    """The keyword options and the caller's sample sets of a RANSAC call, checked: the options into ``opt`` (a ctypes
    structure holding the defaults; ``what`` names the call in an error text) -> the samples as (batch, H, S) int32,
    C-contiguous, None staying None.  ``seed`` must fit 64 unsigned bits; with samples given ``max_iters`` defaults to
    their H and must equal it.  The samples are converted to int32 and (H, S) stands for a batch of one, checked after the
    seed; with ``strict`` (`Backend.homography_ransac`, `Backend.essential_ransac`) they must come as three axes of an
    integer type and are checked first."""

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
