"""numpy restatement of sfmba_triangulate (include/sfmba.h): the n-view DLT through A^T A and a cyclic Jacobi iteration on
the 4x4 matrix, damped Gauss-Newton on the oracle's `compute_residuals` / `jacobian_blocks`, and the verdict.  Written for
the tests: plain loops, one point at a time.  It imports the oracle and changes nothing there."""
import numpy as np

from oracle import ba_oracle as orc

NOT_SELECTED, OK, FEW_VIEWS, AT_INFINITY, BEHIND, LOW_ANGLE, HIGH_ERROR = -1, 0, 1, 2, 3, 4, 5
SWEEPS = 12


def projection_matrices(x, n_cameras, K):
    """M_c = K R_c [I | -T_c] in pixel units, (C, 3, 4)."""
    cams = np.asarray(x[:6 * n_cameras], dtype=np.float64).reshape(n_cameras, 6)
    R = orc.rodrigues(cams[:, :3])
    KR = np.asarray(K, dtype=np.float64) @ R
    return np.concatenate([KR, -(KR @ cams[:, 3:, None])], axis=2)


def cameras_from_projection(M, K):
    """[R | t] = K^-1 M -> the six parameters (rotation vector, centre T = -R^T t) of the bundle-adjustment model."""
    Rt = np.linalg.solve(np.asarray(K, dtype=np.float64), np.asarray(M, dtype=np.float64))
    R, t = Rt[:, :3], Rt[:, 3]
    return np.concatenate([orc.rotvec_from_matrix(R), -R.T @ t])


def dlt_rows(M, uv):
    """The 2n x 4 rows u M3 - M1, v M3 - M2 of n observations (M: (n, 3, 4), uv: (n, 2))."""
    uv = np.asarray(uv, dtype=np.float64)
    a = uv[:, 0, None] * M[:, 2, :] - M[:, 0, :]
    b = uv[:, 1, None] * M[:, 2, :] - M[:, 1, :]
    return np.stack([a, b], axis=1).reshape(-1, 4)


def jacobi_smallest_eigenvector(A):
    """Eigenvector of the smallest eigenvalue of a symmetric 4x4 by cyclic Jacobi rotations (Rutishauser's formulas)."""
    a = np.array(A, dtype=np.float64)
    v = np.eye(4)
    for _ in range(SWEEPS):
        off = np.abs(a[np.triu_indices(4, 1)]).sum()
        if not off > 1e-40 * np.abs(np.diag(a)).sum():
            break
        for p in range(3):
            for q in range(p + 1, 4):
                apq = a[p, q]
                if apq == 0.0:
                    continue
                with np.errstate(over="ignore"):
                    theta = (a[q, q] - a[p, p]) / (2.0 * apq)
                    t = np.copysign(1.0, theta) / (abs(theta) + np.sqrt(theta * theta + 1.0))
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                G = np.eye(4)
                G[p, p] = G[q, q] = c
                G[p, q], G[q, p] = s, -s
                a = G.T @ a @ G
                a[p, q] = a[q, p] = 0.0
                v = v @ G
    return v[:, int(np.argmin(np.diag(a)))]


def linear_point(rows):
    """(X or None, v): the DLT solution of the rows, None when it lies at infinity."""
    v = jacobi_smallest_eigenvector(rows.T @ rows)
    with np.errstate(all="ignore"):
        if not abs(v[3]) > 1e-12 * np.sqrt(v @ v):
            return None, v
        return v[:3] / v[3], v


def svd_point(rows):
    """The same minimiser the way the reference computes it (cv2_lite/triangulate_points.py): last row of V^T."""
    v = np.linalg.svd(rows)[2][-1]
    return v[:3] / v[3]


def _linearise(X, cams, ci, uv, K):
    """sum |r|^2, g, H, depths, errs of one point at X over the observations (cameras ci, pixels uv)."""
    C, n = cams.shape[0], len(ci)
    x = np.concatenate([cams.ravel(), X])
    zeros = np.zeros(n, dtype=np.int64)
    with np.errstate(all="ignore"):
        r, _, Jp = orc.jacobian_blocks(x, C, 1, ci, zeros, uv, K)
        depth = np.einsum("nj,nj->n", orc.rodrigues(cams[:, :3])[ci][:, 2, :], X[None, :] - cams[ci, 3:])
    g = np.einsum("nki,nk->i", Jp, r)
    H = np.einsum("nki,nkj->ij", Jp, Jp)
    return float((r * r).sum()), g, H, depth, np.sqrt((r * r).sum(axis=1))


def gauss_newton_step(X, cams, ci, uv, K):
    """The undamped Gauss-Newton step at X (what the refinement would take next)."""
    _, g, H, _, _ = _linearise(np.asarray(X, dtype=np.float64), cams, ci, uv, K)
    return -np.linalg.solve(H, g)


def cost(X, cams, ci, uv, K):
    return 0.5 * _linearise(np.asarray(X, dtype=np.float64), cams, ci, uv, K)[0]


def widest_angle_deg(X, T):
    """Widest angle between the rays X - T_a, X - T_b over all pairs, as atan2(|a x b|, a . b) in degrees."""
    if len(T) < 2:
        return 0.0
    a = X[None, :] - T
    cr = np.cross(a[:, None, :], a[None, :, :])
    return float(np.degrees(np.arctan2(np.sqrt((cr * cr).sum(axis=2)), a @ a.T)).max())


def stored_runs(point_indices, n_points):
    """(order, ptr): the point-major (stable) order of the observations and the run offsets of the points."""
    pi = np.asarray(point_indices).ravel()
    order = np.argsort(pi, kind="stable")
    return order, np.searchsorted(pi[order], np.arange(n_points + 1))


def triangulate(x, args, select=None, obs_use=None, max_iter=10, min_views=2, xtol=1e-10, min_angle_deg=1.0,
                min_depth=0.0, max_error_px=np.inf):
    """-> dict(points, linear, status, views, iters, rms_err, angle_deg): `linear` (P, 3) holds the DLT point of every
    point that has one (NaN elsewhere), the rest is what sfmba_triangulate returns."""
    C, P, ci, pi, uv, K = args
    x = np.asarray(x, dtype=np.float64)
    ci, pi, uv = np.asarray(ci).ravel(), np.asarray(pi).ravel(), np.asarray(uv, dtype=np.float64)
    cams = x[:6 * C].reshape(C, 6)
    M = projection_matrices(x, C, K)
    order, ptr = stored_runs(pi, P)
    use = np.ones(len(ci), dtype=bool) if obs_use is None else np.asarray(obs_use).ravel() != 0
    sel = np.ones(P, dtype=bool) if select is None else np.asarray(select).ravel() != 0
    out = dict(points=x[6 * C:].reshape(P, 3).copy(), linear=np.full((P, 3), np.nan),
               status=np.full(P, NOT_SELECTED, dtype=np.int32), views=np.zeros(P, dtype=np.int32),
               iters=np.zeros(P, dtype=np.int32), rms_err=np.full(P, np.nan), angle_deg=np.full(P, np.nan))
    for p in np.flatnonzero(sel):
        idx = order[ptr[p]:ptr[p + 1]]
        idx = idx[use[idx]]
        out["views"][p] = len(idx)
        out["status"][p] = FEW_VIEWS
        if len(idx) < max(2, min_views):
            continue
        out["status"][p] = AT_INFINITY
        X, _ = linear_point(dlt_rows(M[ci[idx]], uv[idx]))
        if X is None or not np.all(np.isfinite(X)):
            continue
        out["linear"][p] = X
        c, uvp = ci[idx], uv[idx]
        s, g, H, depth, err = _linearise(X, cams, c, uvp, K)
        if not np.isfinite(s):
            continue
        lam, it = 0.0, 0
        while it < max_iter:
            with np.errstate(all="ignore"):
                try:
                    d = -np.linalg.solve(H + lam * np.diag(np.diag(H)), g)
                except np.linalg.LinAlgError:
                    d = np.full(3, np.nan)
            if np.sqrt(d @ d) <= xtol * (np.sqrt(X @ X) + xtol):          # the step on offer is below the tolerance already
                break
            st, gt, Ht, dt, et = _linearise(X + d, cams, c, uvp, K)
            it += 1
            if st <= s:
                X, s, g, H, depth, err = X + d, st, gt, Ht, dt, et
                lam = 0.1 * lam if lam > 1e-6 else 0.0
                if np.sqrt(d @ d) <= xtol * (np.sqrt(X @ X) + xtol):
                    break
            else:
                if -(g @ d + 0.5 * d @ H @ d) <= 1e-12 * 0.5 * s:       # nothing left that the cost's own rounding would show
                    break
                lam = 1e-3 if lam == 0.0 else 10.0 * lam
        out["iters"][p] = it
        out["rms_err"][p] = np.sqrt(s / len(idx))
        ang = out["angle_deg"][p] = widest_angle_deg(X, cams[c, 3:])
        if depth.min() <= min_depth:
            out["status"][p] = BEHIND
        elif ang < min_angle_deg:
            out["status"][p] = LOW_ANGLE
        elif err.max() > max_error_px:
            out["status"][p] = HIGH_ERROR
        else:
            out["status"][p] = OK
            out["points"][p] = X
    return out
