"""numpy restatement of the two-view calls (include/sfmba.h: sfmba_fundamental_ransac, sfmba_recover_pose): what the
device computes, in the order it is documented, with LAPACK's symmetric eigensolver where the kernels run Jacobi
rotations.  The fixtures measure its distance to the reference (tools/gen_two_view_golden.py); the GPU tests compare the
device with the reference's recorded output and, where no reference output can exist (device-drawn samples, masks,
statuses), with this file."""
import numpy as np

OK, FEW_PAIRS, DEGENERATE, TIE = 0, 1, 2, 3
MASK64 = (1 << 64) - 1
DEG = 57.295779513082320877


# ---- the sample rule -------------------------------------------------------------------------------------------------
def mix(z):
    z &= MASK64
    z ^= z >> 30
    z = (z * 0xbf58476d1ce4e5b9) & MASK64
    z ^= z >> 27
    z = (z * 0x94d049bb133111eb) & MASK64
    z ^= z >> 31
    return z


def draw_sample(seed, e, h, n):
    """The eight distinct positions among n >= 8 used pairs of hypothesis h of the batch's edge e."""
    key = mix(seed ^ mix((e << 32) | h))
    chosen = []
    for j in range(8):
        k = mix((key + (j + 1) * 0x9e3779b97f4a7c15) & MASK64) % (n - j)
        for c in sorted(chosen):
            if k >= c:
                k += 1
        chosen.append(k)
    return chosen


def draw_samples(seed, e, H, n):
    return np.array([draw_sample(seed, e, h, n) for h in range(H)], dtype=np.int32).reshape(H, 8)


# ---- F ------------------------------------------------------------------------------------------------------------------
def normalise(pts):
    """Column means, ONE scale: the standard deviation of all coordinates together (np.std(pts))."""
    mean = pts.mean(axis=0)
    std = np.sqrt(np.mean((pts - pts.mean()) ** 2))
    with np.errstate(divide="ignore", invalid="ignore"):
        T = np.array([[1.0 / std, 0.0, -mean[0] / std], [0.0, 1.0 / std, -mean[1] / std], [0.0, 0.0, 1.0]])
        return (pts - mean) / std, T


def matrix_A(p1, p2):
    return np.column_stack([p2[:, 0] * p1[:, 0], p2[:, 0] * p1[:, 1], p2[:, 0], p2[:, 1] * p1[:, 0], p2[:, 1] * p1[:, 1],
                            p2[:, 1], p1[:, 0], p1[:, 1], np.ones(len(p1))])


def estimate_F(pts1, pts2):
    """The reference's estimate_fundamental_matrix on n >= 8 pairs, not rescaled; NaN where the pairs do not span a scale."""
    n1, T1 = normalise(pts1)
    n2, T2 = normalise(pts2)
    A = matrix_A(n1, n2)
    if not np.isfinite(A).all():
        return np.full((3, 3), np.nan)
    F = np.linalg.eigh(A.T @ A)[1][:, 0].reshape(3, 3)
    v3 = np.linalg.eigh(F.T @ F)[1][:, 0]
    F = F - np.outer(F @ v3, v3)
    return T2.T @ F @ T1


def unit_F(F):
    """Unit Frobenius norm, the entry of largest magnitude (the first of equals) positive."""
    F = np.asarray(F, dtype=np.float64)
    k = int(np.argmax(np.abs(F.ravel())))
    return F / (np.linalg.norm(F) * (-1.0 if F.ravel()[k] < 0 else 1.0))


def distances(F, pts1, pts2):
    """|x2^T F x1| / sqrt(l0^2 + l1^2), l = F x1: the reference's one-sided distance in image 2."""
    x1 = np.column_stack([pts1, np.ones(len(pts1))])
    x2 = np.column_stack([pts2, np.ones(len(pts2))])
    l = x1 @ F.T
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.abs(np.sum(l * x2, axis=1)) / np.sqrt(l[:, 0] ** 2 + l[:, 1] ** 2)


def inliers(F, pts1, pts2, threshold):
    d = distances(F, pts1, pts2)
    with np.errstate(invalid="ignore"):
        return (d < threshold) & np.isfinite(d)


def ransac_edge(pts1, pts2, samples, threshold=1.0, confidence=0.99, refit=False, margin=0.0):
    """One edge over its used pairs with the sample sets `samples` (H, 8) -> dict.  ``near`` (H): a distance of the
    hypothesis lies within `margin` of the threshold (its count may legitimately differ by rounding)."""
    n, H = len(pts1), len(samples)
    out = dict(status=FEW_PAIRS, F=np.zeros((3, 3)), F_refit=np.zeros((3, 3)), mask=np.zeros(n, dtype=bool), inliers=0, best=-1,
               success=False, hyp=np.full(H, -1, dtype=np.int32), near=np.zeros(H, dtype=bool), hyp_F=np.zeros((H, 3, 3)))
    if n < 8:
        return out
    out["status"] = DEGENERATE
    best = None
    for h, idx in enumerate(np.asarray(samples)):
        if len(set(int(k) for k in idx)) < 8:
            continue
        F = estimate_F(pts1[idx], pts2[idx])
        out["hyp_F"][h] = F
        d = distances(F, pts1, pts2)
        with np.errstate(invalid="ignore"):
            m = (d < threshold) & np.isfinite(d)
            out["near"][h] = bool(np.any(np.abs(d - threshold) <= margin))
        out["hyp"][h] = int(m.sum())
        if best is None or out["hyp"][h] > out["hyp"][best]:
            best = h
    if best is None:
        return out
    F = out["hyp_F"][best]
    mask = inliers(F, pts1, pts2, threshold)
    out.update(mask=mask, inliers=int(mask.sum()), best=int(best), success=bool(mask.sum() / n >= confidence))
    if out["hyp"][best] < 8 or not np.isfinite(F).all():        # DEGENERATE: count, h and mask are reported, F is not
        return out
    out.update(status=OK, F=unit_F(F))
    out["F_refit"] = unit_F(estimate_F(pts1[mask], pts2[mask])) if refit else out["F"]
    return out


# ---- pose ---------------------------------------------------------------------------------------------------------------
def decompose(E):
    """The four candidates [(R1, t), (R1, -t), (R2, t), (R2, -t)] with the signs of the header, and (s1, s2)."""
    lam, V = np.linalg.eigh(E.T @ E)
    order = np.argsort(-lam, kind="stable")
    lam, V = lam[order], V[:, order]
    for k in (0, 1):                                             # the component of largest magnitude (the first of equals) positive
        if V[int(np.argmax(np.abs(V[:, k]))), k] < 0:
            V[:, k] = -V[:, k]
    if np.linalg.det(V) < 0:
        V[:, 2] = -V[:, 2]
    s1, s2 = np.linalg.norm(E @ V[:, 0]), np.linalg.norm(E @ V[:, 1])     # (|E v|: good to eps s1, where sqrt(lam) is to sqrt(eps) s1)
    with np.errstate(divide="ignore", invalid="ignore"):
        u1 = E @ V[:, 0] / s1
        u2 = E @ V[:, 1] / s2
        u2 = u2 - (u1 @ u2) * u1
        u2 = u2 / np.linalg.norm(u2)
    u3 = np.cross(u1, u2)
    U = np.column_stack([u1, u2, u3])
    W = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    R1, R2 = U @ W @ V.T, U @ W.T @ V.T
    return [(R1, u3), (R1, -u3), (R2, u3), (R2, -u3)], (s1, s2)


def dlt_points(K, R, t, pts1, pts2):
    """The two-view DLT of triangulate_points_linear2 with M1 = K [I | 0], M2 = K [R | t] -> (n, 3)."""
    M1 = K @ np.hstack([np.eye(3), np.zeros((3, 1))])
    M2 = K @ np.hstack([R, t.reshape(3, 1)])
    X = np.empty((len(pts1), 3))
    for i in range(len(pts1)):
        A = np.array([pts1[i, 0] * M1[2] - M1[0], pts1[i, 1] * M1[2] - M1[1], pts2[i, 0] * M2[2] - M2[0],
                      pts2[i, 1] * M2[2] - M2[1]])
        w = np.linalg.eigh(A.T @ A)[1][:, 0]
        with np.errstate(divide="ignore", invalid="ignore"):
            X[i] = w[:3] / w[3]
    return X


def front_mask(R, t, X, min_depth=0.0):
    d1, d2 = X[:, 2], (X @ R.T + t)[:, 2]
    with np.errstate(invalid="ignore"):
        return (d1 > min_depth) & (d2 > min_depth) & np.isfinite(d1) & np.isfinite(d2)


def ray_angles_deg(R, t, X):
    """The angle at X between the rays to the two camera centres O1 = 0 and O2 = -R^T t, per pair."""
    a, b = X, X + R.T @ t
    return DEG * np.arctan2(np.linalg.norm(np.cross(a, b), axis=1), np.sum(a * b, axis=1))


def reproj_total(K, R, t, X, pts1, pts2):
    p1 = X @ K.T
    p2 = (X @ R.T + t) @ K.T
    with np.errstate(divide="ignore", invalid="ignore"):
        e1 = np.linalg.norm(pts1 - p1[:, :2] / p1[:, 2:3], axis=1)
        e2 = np.linalg.norm(pts2 - p2[:, :2] / p2[:, 2:3], axis=1)
    return float(np.sum(e1 + e2))


def recover_pose_edge(E, pts1, pts2, K, min_depth=0.0):
    """One edge over its used pairs -> dict (status, R, t, mask, X, angle_deg, front, front_all, sum_err)."""
    n = len(pts1)
    out = dict(status=FEW_PAIRS, R=np.zeros((3, 3)), t=np.zeros(3), mask=np.zeros(n, dtype=bool), X=np.full((n, 3), np.nan),
               angle_deg=np.full(n, np.nan), front=0, front_all=np.zeros(4, dtype=np.int32), sum_err=np.nan)
    if n < 1:
        return out
    out["status"] = DEGENERATE
    E = np.asarray(E, dtype=np.float64).reshape(3, 3)
    if not np.isfinite(E).all():
        return out
    cands, (s1, s2) = decompose(E)
    if not s2 > 1e-12 * s1:
        return out
    Xs = [dlt_points(K, R, t, pts1, pts2) for R, t in cands]
    masks = [front_mask(R, t, X, min_depth) for (R, t), X in zip(cands, Xs)]
    counts = np.array([m.sum() for m in masks], dtype=np.int32)
    win = int(np.argmax(counts))                                 # (the first of equal counts)
    R, t = cands[win]
    ang = ray_angles_deg(R, t, Xs[win])
    out.update(status=OK if counts[win] > np.delete(counts, win).max() else TIE, R=R, t=t, mask=masks[win], X=Xs[win],
               angle_deg=np.where(masks[win], ang, np.nan), front=int(counts[win]), front_all=counts,
               sum_err=reproj_total(K, R, t, Xs[win], pts1, pts2))
    return out


# ---- synthetic scenes (the generator's and the tests') --------------------------------------------------------------------
def rodrigues(w):
    th = np.linalg.norm(w)
    if th < 1e-300:
        return np.eye(3)
    k = w / th
    Kx = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + np.sin(th) * Kx + (1.0 - np.cos(th)) * Kx @ Kx


def make_pairs(rng, n, K, noise=0.0, outliers=0.0, angle=0.15, baseline=1.0, t_dir=None):
    """n pairs of a scene 4..9 units deep seen by two cameras (rotation `angle` rad about a random axis, baseline
    `baseline`, along `t_dir` when that is given, else random), `noise` px of Gaussian pixel noise, and a fraction `outliers` of pairs whose second pixel is replaced by
    a uniformly random one -> (pts1, pts2, R, t, is_outlier) with x2 = R x1 + t."""
    w = rng.normal(size=3)
    R = rodrigues(w * (angle / np.linalg.norm(w)))
    t = rng.normal(size=3)
    t[2] *= 0.2
    if t_dir is not None:
        t = np.asarray(t_dir, dtype=np.float64)
    t = t * (baseline / np.linalg.norm(t))
    X = np.stack([rng.uniform(-1.8, 1.8, n), rng.uniform(-1.3, 1.3, n), rng.uniform(4.0, 9.0, n)], axis=1)
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
    return np.ascontiguousarray(p1), np.ascontiguousarray(p2), R, t, bad


def essential_from_pose(R, t):
    tx = np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])
    return tx @ R


def rotation_angle(Ra, Rb):
    """Angle of Ra^T Rb."""
    M = Ra.T @ Rb
    return float(np.arctan2(np.linalg.norm([M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1]]) / 2.0, (np.trace(M) - 1.0) / 2.0))


# ---- the fixtures ---------------------------------------------------------------------------------------------------------
def load_cases(golden_dir):
    """tests/golden/two_view_cases.npz -> (ransac cases, pose cases, K) as lists of dicts."""
    import os
    g = np.load(os.path.join(golden_dir, "two_view_cases.npz"), allow_pickle=False)
    ransac, pose = [], []
    H = g["r_samples"].shape[1]
    bit0 = 0
    packed = g["r_hyp_masks"]
    for k in range(len(g["r_n"])):
        sl = slice(int(g["r_ptr"][k]), int(g["r_ptr"][k + 1]))
        n = int(g["r_n"][k])
        nbytes = (H * n + 7) // 8
        masks = np.unpackbits(packed[bit0:bit0 + nbytes])[:H * n].reshape(H, n).astype(bool)
        bit0 += nbytes
        ransac.append(dict(n=n, noise=float(g["r_noise"][k]), threshold=float(g["r_threshold"][k]), pts1=g["r_pts1"][sl],
                           pts2=g["r_pts2"][sl], samples=g["r_samples"][k], hyp_F=g["r_hyp_F"][k], hyp_masks=masks,
                           hyp_inliers=g["r_hyp_inliers"][k], best=int(g["r_best"][k]), inliers=int(g["r_inliers"][k]),
                           success=bool(g["r_success"][k]), F=g["r_F"][k], F_refit=g["r_F_refit"][k], mask=g["r_mask"][sl]))
    for k in range(len(g["p_n"])):
        sl = slice(int(g["p_ptr"][k]), int(g["p_ptr"][k + 1]))
        pose.append(dict(n=int(g["p_n"][k]), noise=float(g["p_noise"][k]), pts1=g["p_pts1"][sl], pts2=g["p_pts2"][sl],
                         E=g["p_E"][k], R=g["p_R"][k], t=g["p_t"][k], mask=g["p_mask"][sl], err=float(g["p_err"][k])))
    return ransac, pose, g["K"]
