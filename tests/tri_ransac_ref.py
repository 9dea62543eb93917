"""numpy restatement of sfmba_triangulate_ransac (include/sfmba.h), written from its header comment: the pair numbering and
the drawn pairs, the two-view DLT through A^T A and the cyclic Jacobi iteration of triangulate_ref.py, the score, the
best rule, and triangulate_ref.triangulate over the inliers.  Written for the tests: plain loops, one point at a time.

Beside its count a hypothesis carries the flag `close`: a decision inside it was within CLOSE (relative) of going the
other way -- an err^2 against threshold^2, a depth against min_depth, |w3| against its limit, the pair's angle against its
limit -- so that a device result which differs there is no error.  Also here: the contaminated scene the tests share."""
import math

import numpy as np

import triangulate_ref as tr
from pnp_ransac_ref import GOLD, mix

NOT_SELECTED, OK, FEW_VIEWS, AT_INFINITY, BEHIND, LOW_ANGLE, HIGH_ERROR, NO_CONSENSUS = -1, 0, 1, 2, 3, 4, 5, 6
CLOSE = 1e-4
DEFAULTS = dict(threshold=4.0, min_depth=0.0, min_pair_angle_deg=1.0, seed=0, max_pairs=64, min_views=2, refine=1,
                max_iter=10, xtol=1e-10, min_angle_deg=1.0, max_error_px=np.inf)


def pair_count(n):
    return n * (n - 1) // 2 if n >= 2 else 0


def pair_rank(n, i, j):
    return i * (2 * n - i - 1) // 2 + (j - i - 1)


def pair_unrank(n, h):
    """The h-th pair (i < j) of n views in lexicographic order: integer square root of the number counted from the end."""
    r = pair_count(n) - 1 - h
    k = (math.isqrt(8 * r + 1) - 1) // 2
    return n - 2 - k, n - 1 - (r - k * (k + 1) // 2)


def draw2(seed, p, h, n):
    """Two distinct positions among n >= 2, in the order drawn: a function of (seed, point index in the problem, h)."""
    key = mix(int(seed) ^ mix((int(p) << 32) | int(h)))
    first = mix(key + GOLD) % n
    second = mix(key + 2 * GOLD) % (n - 1)
    if second >= first:
        second += 1
    return int(first), int(second)


def hypothesis_pairs(n, p, seed, max_pairs):
    """The pairs (positions among the n used observations) of every hypothesis of point p, in order of h."""
    if pair_count(n) <= max_pairs:
        return [pair_unrank(n, h) for h in range(pair_count(n))]
    return [draw2(seed, p, h, n) for h in range(max_pairs)]


def _near(value, scale):
    return abs(value) <= CLOSE * abs(scale)


def pair_point(Ma, Mb, uva, uvb, solver="jacobi"):
    """(w, X): the homogeneous minimiser of the four DLT rows of two views and X = w[:3] / w[3] (no test applied).
    solver: "jacobi" (the interface's route: A^T A, cyclic Jacobi) or "svd" (an independent route: numpy.linalg.svd)."""
    rows = tr.dlt_rows(np.stack([Ma, Mb]), np.stack([uva, uvb]))
    w = tr.jacobi_smallest_eigenvector(rows.T @ rows) if solver == "jacobi" else np.linalg.svd(rows)[2][-1]
    with np.errstate(all="ignore"):
        return w, w[:3] / w[3]


def project(X, R, T, K):
    """(err-free pixel, depth) of X in the cameras (R, T): pi(K R (X - T)) and the third component of R (X - T)."""
    with np.errstate(all="ignore"):
        q = np.einsum("nij,nj->ni", R, X[None, :] - T)
        px = q @ np.asarray(K, dtype=np.float64).T
        return px[:, :2] / px[:, 2:3], q[:, 2]


def hypothesis(M, R, T, uv, K, a, b, threshold, min_depth, min_pair_angle_deg):
    """One pair (a, b) of the n observations (projection matrices M, rotations R, centres T, pixels uv) ->
    dict(count, valid, X, mask, close)."""
    n = len(uv)
    out = dict(count=0, valid=False, X=None, mask=np.zeros(n, dtype=bool), close=False)
    w, X = pair_point(M[a], M[b], uv[a], uv[b])
    nw = np.sqrt(w @ w)
    if not np.all(np.isfinite(w)):
        return out
    out["close"] |= _near(abs(w[3]) - 1e-12 * nw, 1e-12 * nw)
    if not abs(w[3]) > 1e-12 * nw or not np.all(np.isfinite(X)):
        return out
    pix, depth = project(X, R, T, K)
    dist = np.sqrt(((X[None, :] - T) ** 2).sum(axis=1))
    for k in (a, b):
        out["close"] |= _near(depth[k] - min_depth, dist[k])
    if not (depth[a] > min_depth and depth[b] > min_depth):
        return out
    ra, rb = X - T[a], X - T[b]
    cr = np.cross(ra, rb)
    ang = np.degrees(np.arctan2(np.sqrt(cr @ cr), ra @ rb))
    out["close"] |= _near(ang - min_pair_angle_deg, min_pair_angle_deg)
    if not ang >= min_pair_angle_deg:
        return out
    with np.errstate(all="ignore"):
        e2 = ((pix - uv) ** 2).sum(axis=1)
        thr2 = threshold * threshold
        mask = (e2 < thr2) & (depth > min_depth)
    out["close"] |= bool(np.any(np.abs(e2 - thr2) <= CLOSE * thr2)) or bool(np.any(np.abs(depth - min_depth) <= CLOSE * dist))
    out.update(count=int(mask.sum()), valid=True, X=X, mask=mask)
    return out


def triangulate_ransac(x, args, select=None, obs_use=None, **options):
    """-> dict(points, hyp, inlier_mask (caller's order), status, views, inliers, best, iters, rms_err, angle_deg,
    hyp_inliers (P, H), hyp_close (P, H), hyp_valid (P, H)): what sfmba_triangulate_ransac returns plus the flags."""
    o = dict(DEFAULTS)
    unknown = set(options) - set(o) - {"profile"}
    assert not unknown, unknown
    o.update(options)
    C, P, ci, pi, uv, K = args
    x = np.asarray(x, dtype=np.float64)
    ci, pi, uv = np.asarray(ci).ravel(), np.asarray(pi).ravel(), np.asarray(uv, dtype=np.float64)
    cams = x[:6 * C].reshape(C, 6)
    Rc, Tc = tr.orc.rodrigues(cams[:, :3]), cams[:, 3:]
    M = tr.projection_matrices(x, C, K)
    order, ptr = tr.stored_runs(pi, P)
    use = np.ones(len(ci), dtype=bool) if obs_use is None else np.asarray(obs_use).ravel() != 0
    sel = np.ones(P, dtype=bool) if select is None else np.asarray(select).ravel() != 0
    H, need = int(o["max_pairs"]), max(2, int(o["min_views"]))
    out = dict(hyp=x[6 * C:].reshape(P, 3).copy(), inlier_mask=np.zeros(len(ci), dtype=bool),
               status=np.full(P, NOT_SELECTED, dtype=np.int32), views=np.zeros(P, dtype=np.int32),
               inliers=np.zeros(P, dtype=np.int32), best=np.full(P, -1, dtype=np.int32),
               hyp_inliers=np.full((P, H), -1, dtype=np.int32), hyp_close=np.zeros((P, H), dtype=bool),
               hyp_valid=np.zeros((P, H), dtype=bool))
    for p in np.flatnonzero(sel):
        idx = order[ptr[p]:ptr[p + 1]]
        idx = idx[use[idx]]
        n = len(idx)
        out["views"][p] = n
        out["status"][p] = FEW_VIEWS
        if n < need:
            continue
        c = ci[idx]
        hyps = [hypothesis(M[c], Rc[c], Tc[c], uv[idx], K, a, b, o["threshold"], o["min_depth"], o["min_pair_angle_deg"])
                for a, b in hypothesis_pairs(n, p, o["seed"], H)]
        counts = np.array([r["count"] for r in hyps])
        out["hyp_inliers"][p, :len(hyps)] = counts
        out["hyp_close"][p, :len(hyps)] = [r["close"] for r in hyps]
        out["hyp_valid"][p, :len(hyps)] = [r["valid"] for r in hyps]
        b = int(np.argmax(counts))                               # the first of the largest
        out["best"][p] = b
        out["status"][p] = NO_CONSENSUS
        if hyps[b]["valid"]:
            out["hyp"][p] = hyps[b]["X"]
            out["inlier_mask"][idx] = hyps[b]["mask"]
            out["inliers"][p] = counts[b]
            if counts[b] >= need:
                out["status"][p] = OK
    fin = tr.triangulate(x, args, select=out["status"] == OK, obs_use=out["inlier_mask"],
                         max_iter=int(o["max_iter"]) if o["refine"] else 0, min_views=o["min_views"], xtol=o["xtol"],
                         min_angle_deg=o["min_angle_deg"], min_depth=o["min_depth"], max_error_px=o["max_error_px"])
    reached = out["status"] == OK
    out["status"][reached] = fin["status"][reached]
    out.update(points=fin["points"], iters=fin["iters"], rms_err=fin["rms_err"], angle_deg=fin["angle_deg"],
               linear=fin["linear"])
    return out


def sure_points(ref):
    """Points whose best hypothesis, mask, count and status the restatement pins: no close hypothesis is, or could be level
    with, the best (a close count may be one off; a close validity may turn a count into 0 or back)."""
    P = len(ref["status"])
    sure = np.ones(P, dtype=bool)
    for p in range(P):
        b, close = ref["best"][p], ref["hyp_close"][p]
        if b >= 0 and close.any():
            top = ref["hyp_inliers"][p, b]
            rivals = np.flatnonzero(close)
            # a close hypothesis that is not valid here may be valid there, with any count: it could always win
            if close[b] or np.any(~ref["hyp_valid"][p, rivals]) or ref["hyp_inliers"][p, rivals].max() >= top - 1:
                sure[p] = False
    return sure


# ---- the scene of the tests: 12 cameras on an arc, tracks of 2-12 views, planted wrong observations -----------------------
def arc_scene(n_tracks=400, seed=0, noise=0.5, contaminate=True, lengths=None, n_cameras=12):
    """-> (x, args, planted): cameras c = 0..11 at angle a = 0.12 (c - 6) rad on an arc -- centre (6 sin a, N(0, 0.2),
    6 - 6 cos a), rotation vector (0, -a, 0) + N(0, 0.02) --, points in [-1.5, 1.5] x [-1, 1] x [5, 8], every track a random
    subset of 2-12 cameras (or of lengths[p]), `noise` px of noise; for n >= 4 fewer than (n - 1) // 2 observations are
    displaced by 20-200 px.  planted (N, bool): the displaced observations.  x holds the true cameras and zero points.
    n_cameras: that many cameras on the same arc (angle step 1.44 / n_cameras); a track longer than that sees cameras more
    than once, each time with noise of its own."""
    from sfmba import K_SCEAUX
    rng = np.random.default_rng(seed)
    C = int(n_cameras)
    a = (1.44 / C) * (np.arange(C) - C // 2)
    T = np.stack([6 * np.sin(a), rng.normal(0.0, 0.2, C), 6 - 6 * np.cos(a)], axis=1)
    w = np.stack([np.zeros(C), -a, np.zeros(C)], axis=1) + rng.normal(0.0, 0.02, (C, 3))
    X = np.stack([rng.uniform(-1.5, 1.5, n_tracks), rng.uniform(-1.0, 1.0, n_tracks), rng.uniform(5.0, 8.0, n_tracks)], axis=1)
    lens = rng.integers(2, C + 1, n_tracks) if lengths is None else np.asarray(lengths)
    ci = np.concatenate([np.sort(rng.permutation(C)[:n] if n <= C else rng.integers(0, C, n)) for n in lens]).astype(np.int64)
    pi = np.repeat(np.arange(n_tracks, dtype=np.int64), lens)
    R = tr.orc.rodrigues(w)
    q = np.einsum("nij,nj->ni", R[ci], X[pi] - T[ci]) @ K_SCEAUX.T
    uv = q[:, :2] / q[:, 2:3] + rng.normal(0.0, noise, (len(ci), 2))
    planted = np.zeros(len(ci), dtype=bool)
    if contaminate:
        ptr = np.concatenate([[0], np.cumsum(lens)])
        for p, n in enumerate(lens):
            most = (n - 1) // 2 - 1                              # fewer than (n - 1) // 2
            if n < 4 or most < 1:
                continue
            if rng.random() >= 0.7:                              # (seven eligible tracks in ten carry wrong observations)
                continue
            bad = ptr[p] + rng.permutation(n)[:rng.integers(1, most + 1)]
            ang = rng.uniform(0.0, 2 * np.pi, len(bad))
            uv[bad] += rng.uniform(20.0, 200.0, len(bad))[:, None] * np.stack([np.cos(ang), np.sin(ang)], axis=1)
            planted[bad] = True
    x = np.concatenate([np.hstack([w, T]).ravel(), np.zeros(3 * n_tracks)])
    return x, (C, n_tracks, ci, pi, uv, K_SCEAUX.copy()), planted


# the scenes of tests 1, 2, 7 and 9 (tests/test_gpu_tri_ransac.py) and of tools/gen_tri_ransac_golden.py: arc_scene
# keywords, the call's options, and whether the pixels are rounded to float32 (set_precision(32))
CASES = {
    "arc": dict(scene=dict(n_tracks=400, seed=0), options=dict(), f32=False),
    "arc_h10": dict(scene=dict(n_tracks=150, seed=1), options=dict(max_pairs=10, seed=5), f32=False),
    "arc_f32": dict(scene=dict(n_tracks=150, seed=2), options=dict(), f32=True),
}


def edge_lengths():
    """Track lengths at every switch of k_tri_ransac: n = 2, 3, 4; M = H and M > H for H = 10 (5, 6) and H = 64 (11, 12); the
    lane / wave switch at kStatsLongTrack - 1, itself, + 1; the wave form at one block, one block and one, two and one."""
    from kernel_source import kernel_constant
    L = kernel_constant("kStatsLongTrack")
    return [2, 3, 4, 5, 6, 11, 12, L - 1, L, L + 1, 64, 65, 129]


def edge_scene():
    """arc_scene keywords of the edge scene: 40 cameras, 45 tracks of 2-4 views, every third one of edge_lengths()."""
    lens = [2, 3, 4] * 15
    for k, n in enumerate(edge_lengths()):
        lens[3 * k + 1] = n
    return dict(n_tracks=len(lens), seed=7, lengths=lens, n_cameras=40)


# the edge scene with every option set its tests run against the restatement (`also`: their pairs count for the bounds too)
EDGE_OPTIONS = [dict(max_pairs=64, seed=11), dict(max_pairs=10, seed=11), dict(max_pairs=1, seed=11), dict(max_pairs=20, seed=4)]
CASES["edges"] = dict(scene=edge_scene(), options=EDGE_OPTIONS[0], also=EDGE_OPTIONS[1:], f32=False)
CASES["edges_f32"] = dict(scene=edge_scene(), options=EDGE_OPTIONS[3], f32=True)


def case_inputs(name):
    """-> (x, args, planted, options) of CASES[name]; with f32 the pixels are the float32-rounded ones, as stored."""
    case = CASES[name]
    x, args, planted = arc_scene(**case["scene"])
    if case["f32"]:
        args = args[:4] + (args[4].astype(np.float32).astype(np.float64),) + args[5:]
    return x, args, planted, dict(case["options"])


def _route_distances(x, args, ref, options):
    """Largest relative distance of the Jacobi route to the SVD route over every valid pair point of `ref` and over the
    n-view linear point of every inlier set that has one -> (pair, linear, pairs compared)."""
    C, P, ci, pi, uv, K = args
    lin = tr.triangulate(x, args, select=np.isin(ref["status"], (OK, BEHIND, LOW_ANGLE, HIGH_ERROR)), obs_use=ref["inlier_mask"],
                         max_iter=0)
    M = tr.projection_matrices(x, C, K)
    order, ptr = tr.stored_runs(pi, P)
    d_pair = d_lin = 0.0
    n_pairs = 0
    for p in range(P):
        idx = order[ptr[p]:ptr[p + 1]]
        pairs = hypothesis_pairs(len(idx), p, options.get("seed", 0), options.get("max_pairs", DEFAULTS["max_pairs"]))
        for h, (a, b) in enumerate(pairs):
            if not ref["hyp_valid"][p, h]:
                continue
            Xj = pair_point(M[ci[idx[a]]], M[ci[idx[b]]], uv[idx[a]], uv[idx[b]])[1]
            Xs = pair_point(M[ci[idx[a]]], M[ci[idx[b]]], uv[idx[a]], uv[idx[b]], solver="svd")[1]
            d_pair = max(d_pair, float(np.abs(Xj - Xs).max() / max(1.0, np.abs(Xs).max())))
            n_pairs += 1
        inl = idx[ref["inlier_mask"][idx]]
        if np.all(np.isfinite(lin["linear"][p])):
            Xs = tr.svd_point(tr.dlt_rows(M[ci[inl]], uv[inl]))
            d_lin = max(d_lin, float(np.abs(lin["linear"][p] - Xs).max() / max(1.0, np.abs(Xs).max())))
    return d_pair, d_lin, n_pairs


def measure_case(name):
    """What tests/golden/tri_ransac_bounds.json records of a case, from the restatement alone (no device): the share of
    close hypotheses, the distance of the Jacobi route to the SVD route over every valid pair point and over the linear
    point of every inlier set (the largest over the case's option sets), the planted-truth recovery, and what the plain
    all-view triangulation with max_error_px = 4 makes of the contaminated tracks.  -> (record, ref)"""
    x, args, planted, options = case_inputs(name)
    C, P, ci, pi, uv, K = args
    ref = triangulate_ransac(x, args, **options)
    exists = ref["hyp_inliers"] >= 0
    order, ptr = tr.stored_runs(pi, P)
    d_pair, d_lin, n_pairs = _route_distances(x, args, ref, options)
    for extra in CASES[name].get("also", []):
        a, b, n = _route_distances(x, args, triangulate_ransac(x, args, **extra), extra)
        d_pair, d_lin, n_pairs = max(d_pair, a), max(d_lin, b), n_pairs + n
    contaminated = np.flatnonzero(np.bincount(pi[planted], minlength=P) > 0)
    recovered = [p for p in contaminated if ref["status"][p] == OK and
                 np.array_equal(ref["inlier_mask"][order[ptr[p]:ptr[p + 1]]], ~planted[order[ptr[p]:ptr[p + 1]]])]
    plain = tr.triangulate(x, args, max_error_px=4.0)["status"][contaminated]
    rec = dict(hypotheses=int(exists.sum()), close=int(ref["hyp_close"].sum()),
               close_share=float(ref["hyp_close"].sum() / exists.sum()), sure_points=int(sure_points(ref).sum()),
               pairs_compared=n_pairs, pair_measured_rel=d_pair, final_linear_measured_rel=d_lin,
               contaminated_tracks=int(len(contaminated)), recovered=int(len(recovered)),
               recovered_share=float(len(recovered) / max(1, len(contaminated))), n_ok=int((ref["status"] == OK).sum()),
               plain_high_error=int((plain == HIGH_ERROR).sum()), plain_behind=int((plain == BEHIND).sum()),
               plain_ok=int((plain == OK).sum()))
    return rec, ref
