"""Sequential restatement of sfmba_plan_views and sfmba_assemble_problem / sfmba_get_assembled (include/sfmba.h,
DESIGN.md section 25) and generators for their tests.

Both functions walk the tracks one observation at a time in plain Python, from a `Tracks` object or from what
`track_ref.build_tracks_ref` returns (then with the build's ``img_ptr``), plus the two masks.  Sizes at which the kernels
change their path are read from the source, so the edge cases follow the code."""
import os
import re

import numpy as np

import track_ref as tr
from conftest import ROOT

VIEW_FIELDS = ("trk_reg_views", "img_tracks", "img_known", "img_gain")
SUB_FIELDS = ("cam_of", "pt_of", "camera_indices", "point_indices", "obs_feat")


def plan_constant(name):
    src = open(os.path.join(ROOT, "sfm-python_amd", "csrc", "plan_kernels.hpp")).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1))


def tables(tracks, img_ptr=None):
    """(img_ptr, feat_track, track_ptr, track_feat, track_image) as lists, from a Tracks object or a build_tracks_ref dict."""
    if isinstance(tracks, dict):
        src = [img_ptr] + [tracks[k] for k in tr.FIELDS]
    else:
        src = [tracks.img_ptr] + [getattr(tracks, k) for k in tr.FIELDS]
    return [np.asarray(a).tolist() for a in src]


def plan_views_ref(tracks, cam_reg, trk_known, img_ptr=None):
    img_ptr, feat_track, track_ptr, _, track_image = tables(tracks, img_ptr)
    reg = [int(bool(v)) for v in np.asarray(cam_reg).tolist()]
    known = [bool(v) for v in np.asarray(trk_known).tolist()]
    n_images, n_tracks = len(img_ptr) - 1, len(track_ptr) - 1
    assert len(reg) == n_images and len(known) == n_tracks
    views = [sum(reg[track_image[k]] for k in range(track_ptr[t], track_ptr[t + 1])) for t in range(n_tracks)]
    img_tracks, img_known, img_gain = [0] * n_images, [0] * n_images, [0] * n_images
    for i in range(n_images):
        for f in range(img_ptr[i], img_ptr[i + 1]):
            t = feat_track[f]
            if t < 0:
                continue
            img_tracks[i] += 1
            if known[t]:
                img_known[i] += 1
            elif views[t] - reg[i] >= 1:
                img_gain[i] += 1
    ready = sum(1 for t in range(n_tracks) if not known[t] and views[t] >= 2)
    return dict(trk_reg_views=np.array(views, dtype=np.int32).reshape(-1), img_tracks=np.array(img_tracks, dtype=np.int32).reshape(-1),
                img_known=np.array(img_known, dtype=np.int32).reshape(-1), img_gain=np.array(img_gain, dtype=np.int32).reshape(-1),
                totals=dict(registered=sum(reg), known=sum(known), ready=ready))


def assemble_ref(tracks, cam_use, trk_use, min_views=2, pts=None, img_ptr=None):
    """``pts``: (N, 2) pixels of all features, or None -> ``points_2d`` None."""
    img_ptr, _, track_ptr, track_feat, track_image = tables(tracks, img_ptr)
    cam = [bool(v) for v in np.asarray(cam_use).tolist()]
    use = [bool(v) for v in np.asarray(trk_use).tolist()]
    assert len(cam) == len(img_ptr) - 1 and len(use) == len(track_ptr) - 1 and min_views >= 1
    pt_of, obs = [], []                                          # obs: (image, sub-point, feature)
    for t in range(len(track_ptr) - 1):
        used = [k for k in range(track_ptr[t], track_ptr[t + 1]) if use[t] and cam[track_image[k]]]
        if len(used) < min_views:
            continue
        obs += [(track_image[k], len(pt_of), track_feat[k]) for k in used]
        pt_of.append(t)
    cam_of = sorted({o[0] for o in obs})
    number = {image: c for c, image in enumerate(cam_of)}
    obs_feat = np.array([o[2] for o in obs], dtype=np.int32).reshape(-1)
    return dict(cam_of=np.array(cam_of, dtype=np.int32).reshape(-1), pt_of=np.array(pt_of, dtype=np.int32).reshape(-1),
                camera_indices=np.array([number[o[0]] for o in obs], dtype=np.int64).reshape(-1),
                point_indices=np.array([o[1] for o in obs], dtype=np.int64).reshape(-1), obs_feat=obs_feat,
                points_2d=None if pts is None else np.ascontiguousarray(np.asarray(pts, dtype=np.float64).reshape(-1, 2)[obs_feat]),
                counts=dict(cameras=len(cam_of), points=len(pt_of), observations=len(obs)))


# ---- generators --------------------------------------------------------------------------------------------------------
def exact_tracks(rng, rows, M, n_tracks):
    """A `tr.random_batch` scene cut down to exactly ``n_tracks`` tracks -> (batch, pair_use): the pairs of its first
    ``n_tracks`` components are used (a component is closed under its pairs), built with ``conflicts=1``."""
    batch = tr.random_batch(rng, rows, M)
    ref = tr.build_tracks_ref(*batch, conflicts=1)
    assert ref["counts"]["tracks"] >= n_tracks, (ref["counts"]["tracks"], n_tracks)
    g = tr.global_pairs(*batch)
    return batch, ref["feat_track"][g[:, 0]] < n_tracks


def pixels(rng, img_ptr):
    """A list of (n_i, 2) pixel arrays, one per image, with many different bit patterns."""
    rows = np.diff(np.asarray(img_ptr))
    return [np.ascontiguousarray(rng.normal(500.0, 300.0, (int(n), 2)) * 10.0 ** rng.integers(-3, 4, (int(n), 1))) for n in rows]
