"""numpy restatement of the homography call (include/sfmba.h: sfmba_homography_ransac), written from the header: what the
device computes, in the order it is documented, with LAPACK's symmetric eigensolver where the kernels run Jacobi
rotations.  There is no reference code for H; the GPU tests compare the device with this file."""
import numpy as np

import two_view_ref as tv
from two_view_ref import MASK64, make_pairs, mix, normalise

OK, FEW_PAIRS, DEGENERATE = 0, 1, 2


# ---- the sample rule -------------------------------------------------------------------------------------------------
def draw_sample4(seed, e, h, n):
    """The four distinct positions among n >= 4 used pairs of hypothesis h of the batch's edge e."""
    key = mix(seed ^ mix((e << 32) | h))
    chosen = []
    for j in range(4):
        k = mix((key + (j + 1) * 0x9e3779b97f4a7c15) & MASK64) % (n - j)
        for c in sorted(chosen):
            if k >= c:
                k += 1
        chosen.append(k)
    return chosen


def draw_samples4(seed, e, H, n):
    return np.array([draw_sample4(seed, e, h, n) for h in range(H)], dtype=np.int32).reshape(H, 4)


# ---- H -------------------------------------------------------------------------------------------------------------------
def rows(p1, p2):
    """The 2n x 9 matrix of the normalised pairs (x, y) -> (u, v): all first rows, then all second rows."""
    x, y, u, v = p1[:, 0], p1[:, 1], p2[:, 0], p2[:, 1]
    o, z = np.ones(len(p1)), np.zeros(len(p1))
    first = np.column_stack([-x, -y, -o, z, z, z, u * x, u * y, u])
    second = np.column_stack([z, z, z, -x, -y, -o, v * x, v * y, v])
    return np.concatenate([first, second])


def estimate_parts(pts1, pts2):
    """-> (A, T1, inverse of T2) of the estimate on n >= 4 pairs."""
    n1, T1 = normalise(pts1)
    n2, T2 = normalise(pts2)
    with np.errstate(divide="ignore", invalid="ignore"):
        s2 = 1.0 / T2[0, 0]
        T2inv = np.array([[s2, 0.0, -T2[0, 2] * s2], [0.0, s2, -T2[1, 2] * s2], [0.0, 0.0, 1.0]])
    return rows(n1, n2), T1, T2inv


def estimate_H(pts1, pts2):
    """The four-point (or n-point) DLT of the header, not rescaled; NaN where the pairs do not span a scale."""
    A, T1, T2inv = estimate_parts(pts1, pts2)
    if not (np.isfinite(A).all() and np.isfinite(T2inv).all() and np.isfinite(T1).all()):
        return np.full((3, 3), np.nan)
    Hn = np.linalg.eigh(A.T @ A)[1][:, 0].reshape(3, 3)
    return T2inv @ Hn @ T1


def unit_H(H):
    """Unit Frobenius norm, the entry of largest magnitude (the first of equals) positive."""
    return tv.unit_F(H)


def distances_sq(H, pts1, pts2):
    """(q0/q2 - x2)^2 + (q1/q2 - y2)^2 with q = H (x1, y1, 1): the squared one-sided transfer distance in image 2."""
    q = np.column_stack([pts1, np.ones(len(pts1))]) @ H.T
    with np.errstate(divide="ignore", invalid="ignore"):
        return (q[:, 0] / q[:, 2] - pts2[:, 0]) ** 2 + (q[:, 1] / q[:, 2] - pts2[:, 1]) ** 2


def inliers(H, pts1, pts2, threshold):
    d2 = distances_sq(H, pts1, pts2)
    with np.errstate(invalid="ignore"):
        return (d2 < threshold * threshold) & np.isfinite(d2)


def near_threshold(H, pts1, pts2, threshold, margin):
    """A distance (not squared) of H lies within `margin` of the threshold."""
    with np.errstate(invalid="ignore"):
        return bool(np.any(np.abs(np.sqrt(distances_sq(H, pts1, pts2)) - threshold) <= margin))


def ransac_edge(pts1, pts2, samples, threshold=1.0, confidence=0.99, refit=False, margin=0.0):
    """One edge over its used pairs with the sample sets `samples` (H, 4) -> dict.  ``near`` (H): a distance of the
    hypothesis lies within `margin` of the threshold (its count may legitimately differ by rounding); ``near_refit``:
    the same of H_refit."""
    n, nh = len(pts1), len(samples)
    out = dict(status=FEW_PAIRS, H=np.zeros((3, 3)), H_refit=np.zeros((3, 3)), mask=np.zeros(n, dtype=bool),
               refit_mask=np.zeros(n, dtype=bool), inliers=0, refit_inliers=0, best=-1, success=False,
               hyp=np.full(nh, -1, dtype=np.int32), near=np.zeros(nh, dtype=bool), near_refit=False, hyp_H=np.zeros((nh, 3, 3)))
    if n < 4:
        return out
    out["status"] = DEGENERATE
    best = None
    for h, idx in enumerate(np.asarray(samples)):
        if len(set(int(k) for k in idx)) < 4:
            continue
        H = estimate_H(pts1[idx], pts2[idx])
        out["hyp_H"][h] = H
        out["near"][h] = near_threshold(H, pts1, pts2, threshold, margin)
        out["hyp"][h] = int(inliers(H, pts1, pts2, threshold).sum())
        if best is None or out["hyp"][h] > out["hyp"][best]:
            best = h
    if best is None:
        return out
    H = out["hyp_H"][best]
    mask = inliers(H, pts1, pts2, threshold)
    out.update(mask=mask, refit_mask=mask, inliers=int(mask.sum()), refit_inliers=int(mask.sum()), best=int(best),
               success=bool(mask.sum() / n >= confidence))
    if out["hyp"][best] < 4 or not np.isfinite(H).all():        # DEGENERATE: count, h and mask are reported, H is not
        return out
    out.update(status=OK, H=unit_H(H), H_refit=unit_H(H))
    if refit:
        Hr = estimate_H(pts1[mask], pts2[mask])
        Hr = unit_H(Hr) if np.isfinite(Hr).all() else out["H"]
        rmask = inliers(Hr, pts1, pts2, threshold)
        out.update(H_refit=Hr, refit_mask=rmask, refit_inliers=int(rmask.sum()),
                   near_refit=near_threshold(Hr, pts1, pts2, threshold, margin))
    return out


def estimate_tolerance(pts1, pts2):
    """The bound of a device H (unit norm) against this file's on the same pairs: the null vector h of A moves by
    |d(A^T A)| / (l2 - l1), with |d(A^T A)| a few eps l9 from forming the sums in another order, and the unit-norm
    H = T2^-1 Hn T1 / |T2^-1 Hn T1| by at most 2 |T1| |T2^-1| / |T2^-1 Hn T1| times that."""
    A, T1, T2inv = estimate_parts(pts1, pts2)
    lam, vec = np.linalg.eigh(A.T @ A)
    H = T2inv @ vec[:, 0].reshape(3, 3) @ T1
    eps = np.finfo(np.float64).eps
    return 64 * eps * lam[-1] / (lam[1] - lam[0]) * 2.0 * np.linalg.norm(T1, 2) * np.linalg.norm(T2inv, 2) / np.linalg.norm(H)


# ---- synthetic scenes ------------------------------------------------------------------------------------------------------
def planar_pairs(rng, n, K, noise=0.0, outliers=0.0, baseline=1.0, angle=0.15):
    """n pairs of points on a tilted plane 4..9 units deep seen by two cameras (rotation `angle` rad about a random
    axis, baseline `baseline`; 0 gives the pure rotation), `noise` px of Gaussian pixel noise, a fraction `outliers` of
    pairs whose second pixel is replaced by a uniformly random one -> (pts1, pts2, H, R, t, is_outlier) with H the
    homography of the exact pixels, x2 ~ H x1."""
    w = rng.normal(size=3)
    R = tv.rodrigues(w * (angle / np.linalg.norm(w)))
    t = rng.normal(size=3)
    t[2] *= 0.2
    t = t * (baseline / np.linalg.norm(t))
    # the plane nrm . X = d through (0, 0, 6.5); its slopes keep the depth inside 4..9 over the field of view
    a, b = rng.uniform(-0.6, 0.6), rng.uniform(-0.6, 0.6)
    x, y = rng.uniform(-1.8, 1.8, n), rng.uniform(-1.3, 1.3, n)
    X = np.stack([x, y, 6.5 + a * x + b * y], axis=1)
    nrm, d = np.array([-a, -b, 1.0]), 6.5
    Hm = K @ (R + np.outer(t, nrm) / d) @ np.linalg.inv(K)
    p1 = X @ K.T
    p2 = (X @ R.T + t) @ K.T
    p1, p2 = p1[:, :2] / p1[:, 2:3], p2[:, :2] / p2[:, 2:3]
    p1 = p1 + noise * rng.normal(size=(n, 2))
    p2 = p2 + noise * rng.normal(size=(n, 2))
    bad = np.zeros(n, dtype=bool)
    n_bad = int(round(outliers * n))
    if n_bad:
        bad[rng.choice(n, n_bad, replace=False)] = True
        p2[bad] = np.stack([rng.uniform(0.0, 2.0 * K[0, 2], n_bad), rng.uniform(0.0, 2.0 * K[1, 2], n_bad)], axis=1)
    return np.ascontiguousarray(p1), np.ascontiguousarray(p2), Hm, R, t, bad
