"""numpy restatement of the similarity call (include/sfmba.h: sfmba_similarity_ransac), written from the header: what the
device computes, in the order it is documented, with LAPACK's symmetric eigensolver where the kernels run Jacobi
rotations.  The GPU tests compare the device with this file; tests/test_host_similarity.py compares this file's Horn
estimate with the oracle's Umeyama (SVD) one."""
import numpy as np

from two_view_ref import MASK64, mix

OK, FEW_PAIRS, DEGENERATE = 0, 1, 2
EIGEN_GAP = 1e-9
EPS = np.finfo(np.float64).eps


# ---- the sample rule -------------------------------------------------------------------------------------------------
def draw_sample3(seed, e, h, n):
    """The three distinct positions among n >= 3 used pairs of hypothesis h of the batch's set e."""
    key = mix(seed ^ mix((e << 32) | h))
    chosen = []
    for j in range(3):
        k = mix((key + (j + 1) * 0x9e3779b97f4a7c15) & MASK64) % (n - j)
        for c in sorted(chosen):
            if k >= c:
                k += 1
        chosen.append(k)
    return chosen


def draw_samples3(seed, e, H, n):
    return np.array([draw_sample3(seed, e, h, n) for h in range(H)], dtype=np.int32).reshape(H, 3)


# ---- Horn's closed form ----------------------------------------------------------------------------------------------
def horn_matrix(S):
    """The symmetric 4 x 4 matrix N of the header from S[i, j] = sum a'_i b'_j."""
    (Sxx, Sxy, Sxz), (Syx, Syy, Syz), (Szx, Szy, Szz) = S
    return np.array([[Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx],
                     [Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz],
                     [Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy],
                     [Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz]])


def rotation_of(q):
    w, x, y, z = q
    return np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]])


def horn_parts(src, dst):
    """-> (am, bm, S, saa, N) of n >= 1 pairs."""
    src, dst = np.asarray(src, dtype=np.float64).reshape(-1, 3), np.asarray(dst, dtype=np.float64).reshape(-1, 3)
    am, bm = src.sum(axis=0) / len(src), dst.sum(axis=0) / len(dst)
    ac, bc = src - am, dst - bm
    S = ac.T @ bc
    return am, bm, S, float((ac * ac).sum()), horn_matrix(S)


def horn(src, dst):
    """The estimate of the header on n >= 3 pairs -> (s, R, t), or None where the header says NO SOLUTION."""
    am, bm, S, saa, N = horn_parts(src, dst)
    if not np.isfinite(N).all():
        return None
    lam, vec = np.linalg.eigh(N)                                 # ascending: l1 = lam[3]
    if not lam[3] - lam[2] > EIGEN_GAP * (lam[3] - lam[0]):
        return None
    q = vec[:, 3] / np.linalg.norm(vec[:, 3])
    R = rotation_of(q)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = float((R.T * S).sum() / saa)
    if not saa > 0.0 or not s > 0.0:
        return None
    t = bm - s * (R @ am)
    if not (np.isfinite(s) and np.isfinite(R).all() and np.isfinite(t).all()):
        return None
    return s, R, t


def distances_sq(sim, src, dst):
    """|s R a + t - b|^2 of every pair."""
    s, R, t = sim
    d = s * (np.asarray(src) @ R.T) + t - np.asarray(dst)
    return (d * d).sum(axis=1)


def inliers(sim, src, dst, threshold):
    d2 = distances_sq(sim, src, dst)
    with np.errstate(invalid="ignore"):
        return (d2 < threshold * threshold) & np.isfinite(d2)


def near_threshold(sim, src, dst, threshold, margin):
    """A distance (not squared) of the similarity lies within `margin` of the threshold."""
    with np.errstate(invalid="ignore"):
        return bool(np.any(np.abs(np.sqrt(distances_sq(sim, src, dst)) - threshold) <= margin))


def flat(sim):
    """(s, R, t) -> the 13 doubles of the call."""
    return np.concatenate([[sim[0]], np.asarray(sim[1]).ravel(), np.asarray(sim[2]).ravel()])


def ransac_set(src, dst, samples, threshold, confidence=0.99, refit=False, margin=0.0):
    """One set over its used pairs with the sample sets `samples` (H, 3) -> dict.  ``sim`` / ``sim_refit``: (s, R, t) or
    None; ``near`` (H): a distance of the hypothesis lies within `margin` of the threshold (its count may legitimately
    differ by rounding); ``near_refit``: the same of the refit."""
    src, dst = np.asarray(src, dtype=np.float64).reshape(-1, 3), np.asarray(dst, dtype=np.float64).reshape(-1, 3)
    n, nh = len(src), len(samples)
    out = dict(status=FEW_PAIRS, sim=None, sim_refit=None, mask=np.zeros(n, dtype=bool), refit_mask=np.zeros(n, dtype=bool),
               inliers=0, refit_inliers=0, best=-1, success=False, hyp=np.full(nh, -1, dtype=np.int32),
               near=np.zeros(nh, dtype=bool), near_refit=False, hyp_sim=[None] * nh)
    if n < 3:
        return out
    out["status"] = DEGENERATE
    best = None
    for h, idx in enumerate(np.asarray(samples)):
        if len(set(int(k) for k in idx)) < 3:
            continue
        sim = horn(src[idx], dst[idx])
        out["hyp_sim"][h] = sim
        out["hyp"][h] = 0
        if sim is not None:
            out["near"][h] = near_threshold(sim, src, dst, threshold, margin)
            out["hyp"][h] = int(inliers(sim, src, dst, threshold).sum())
        if best is None or out["hyp"][h] > out["hyp"][best]:
            best = h
    if best is None:
        return out
    sim = out["hyp_sim"][best]
    mask = inliers(sim, src, dst, threshold) if sim is not None else np.zeros(n, dtype=bool)
    out.update(mask=mask, refit_mask=mask, inliers=int(mask.sum()), refit_inliers=int(mask.sum()), best=int(best),
               success=bool(mask.sum() / n >= confidence))
    if sim is None or mask.sum() < 3:                            # DEGENERATE: count, h and mask are reported
        return out
    out.update(status=OK, sim=sim, sim_refit=sim)
    if refit:
        sr = horn(src[mask], dst[mask])
        sr = sr if sr is not None else sim
        rmask = inliers(sr, src, dst, threshold)
        out.update(sim_refit=sr, refit_mask=rmask, refit_inliers=int(rmask.sum()),
                   near_refit=near_threshold(sr, src, dst, threshold, margin))
    return out


def estimate_tolerance(src, dst):
    """The bounds (ds, dR, dt) of a device estimate against this file's on the same pairs, entry by entry: the unit
    quaternion moves by |dN| / (l1 - l2) with |dN| = 64 eps |N|_F from forming the sums in another order and from the
    Jacobi rotations; R is quadratic in q, a turn by the angle dR = 2 dq (its entries and its 2-norm move by that much,
    its Frobenius norm by sqrt 2 dR); s = sum_ij R_ji S_ij / saa moves by |S|_F sqrt 2 dR / saa + 64 eps s;
    t = bm - s R am by |bm| eps + s dR |am| + ds |am|."""
    am, bm, S, saa, N = horn_parts(src, dst)
    lam = np.linalg.eigvalsh(N)
    s = horn(src, dst)[0]
    dq = 64 * EPS * np.linalg.norm(N) / (lam[3] - lam[2])
    dR = 2.0 * dq
    ds = np.linalg.norm(S) * np.sqrt(2.0) * dR / saa + 64 * EPS * s
    dt = np.linalg.norm(bm) * EPS + s * dR * np.linalg.norm(am) + ds * np.linalg.norm(am)
    return ds, dR, dt


def tolerance_ratio(got, want, src, dst):
    """The largest |got - want| / bound over s, R and t (each (s, R, t)) under estimate_tolerance(src, dst)."""
    ds, dR, dt = estimate_tolerance(src, dst)
    return max(abs(got[0] - want[0]) / ds, np.abs(np.asarray(got[1]) - want[1]).max() / dR,
               np.abs(np.asarray(got[2]).ravel() - want[2]).max() / dt)


# ---- synthetic sets ----------------------------------------------------------------------------------------------------
def rodrigues(w):
    th = np.linalg.norm(w)
    if th == 0.0:
        return np.eye(3)
    k = np.asarray(w) / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


def similar_sets(rng, n, noise=0.0, outliers=0.0, spread=8.0, scale=None, angle=None, displace=8.0):
    """n pairs: src uniform in a cube of side 2 `spread` about a random centre, dst = s R src + t + `noise` x N(0, 1) per
    coordinate (s in 0.5 .. 3 unless `scale`, a rotation of `angle` rad (None: 0.2 .. 3) about a random axis, t of a few
    units), a fraction `outliers` of the dst points displaced by up to +-`displace` per coordinate and by at least a
    quarter of it along one -> (src, dst, (s, R, t), is_outlier)."""
    src = rng.uniform(-spread, spread, (n, 3)) + rng.normal(size=3) * 3.0
    s = float(rng.uniform(0.5, 3.0)) if scale is None else float(scale)
    w = rng.normal(size=3)
    R = rodrigues(w * ((rng.uniform(0.2, 3.0) if angle is None else angle) / np.linalg.norm(w)))
    t = rng.normal(size=3) * 5.0
    dst = s * (src @ R.T) + t + noise * rng.normal(size=(n, 3))
    bad = np.zeros(n, dtype=bool)
    n_bad = int(round(outliers * n))
    if n_bad:
        bad[rng.choice(n, n_bad, replace=False)] = True
        d = rng.uniform(-displace, displace, (n_bad, 3))
        d[:, 0] = np.where(np.abs(d[:, 0]) < 0.25 * displace, np.copysign(0.25 * displace, d[:, 0]), d[:, 0])
        dst[bad] += d
    return np.ascontiguousarray(src), np.ascontiguousarray(dst), (s, R, t), bad
