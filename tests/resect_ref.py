"""numpy restatement of sfmba_resect (include/sfmba.h): the n-point DLT through the forty sums of A^T A and a cyclic Jacobi
iteration on the 12x12 matrix, R = M (M^T M)^(-1/2) by a 3x3 Jacobi, t scaled by the mean singular value, damped
Gauss-Newton over (omega, T) on the oracle's `jacobian_blocks`, and the verdict.  Written for the tests: plain loops, one
camera at a time.  It imports the oracle and changes nothing there."""
import numpy as np

from oracle import ba_oracle as orc

NOT_SELECTED, OK, FEW_VIEWS, DEGENERATE, BEHIND, HIGH_ERROR = -1, 0, 1, 2, 3, 4
SWEEPS12, SWEEPS3 = 30, 12
TRIU4 = np.triu_indices(4)


def dlt_rows(X, uvn):
    """The 2n x 12 rows [P, 0, -u P], [0, P, -v P] of n correspondences (X: (n, 3) points, uvn: (n, 2) normalised pixels)."""
    n = len(X)
    P = np.concatenate([np.asarray(X, dtype=np.float64), np.ones((n, 1))], axis=1)
    A = np.zeros((2 * n, 12))
    A[0::2, 0:4] = P
    A[0::2, 8:12] = -uvn[:, 0, None] * P
    A[1::2, 4:8] = P
    A[1::2, 8:12] = -uvn[:, 1, None] * P
    return A


def normalise_pixels(uv, K):
    """K^-1 (u, v, 1), first two rows, as the reference does it (no division by the third)."""
    Kinv = np.linalg.inv(np.asarray(K, dtype=np.float64))
    uv = np.asarray(uv, dtype=np.float64)
    return uv @ Kinv[:2, :2].T + Kinv[:2, 2]


def forty_sums(X, uvn):
    """S, S_u, S_v, S_w (each the upper triangle of a symmetric 4x4, row by row): sums over the correspondences in order."""
    s = np.zeros((4, 10))
    for k in range(len(X)):
        P = np.array([X[k, 0], X[k, 1], X[k, 2], 1.0])
        pp = np.outer(P, P)[TRIU4]
        u, v = uvn[k]
        s[0] += pp
        s[1] += u * pp
        s[2] += v * pp
        s[3] += (u * u + v * v) * pp
    return s


def _sym4(t):
    m = np.zeros((4, 4))
    m[TRIU4] = t
    return m + np.triu(m, 1).T


def ata_from_sums(s):
    """A^T A = [[S, 0, -S_u], [0, S, -S_v], [-S_u, -S_v, S_w]]."""
    S, Su, Sv, Sw = (_sym4(t) for t in s)
    Z = np.zeros((4, 4))
    return np.block([[S, Z, -Su], [Z, S, -Sv], [-Su, -Sv, Sw]])


def jacobi_eigh(A, sweeps):
    """(diagonal, V) of a symmetric matrix by cyclic Jacobi rotations over the pairs (0,1), (0,2), ..., (n-2,n-1)
    (Rutishauser's formulas), until the off-diagonal part is 1e-40 of the diagonal; eigenvectors in the columns of V."""
    a = np.array(A, dtype=np.float64)
    n = a.shape[0]
    v = np.eye(n)
    iu = np.triu_indices(n, 1)
    for _ in range(sweeps):
        off = np.abs(a[iu]).sum()
        if not off > 1e-40 * np.abs(np.diag(a)).sum():
            break
        for p in range(n - 1):
            for q in range(p + 1, n):
                apq = a[p, q]
                if apq == 0.0:
                    continue
                with np.errstate(over="ignore"):
                    theta = (a[q, q] - a[p, p]) / (2.0 * apq)
                    t = np.copysign(1.0, theta) / (abs(theta) + np.sqrt(theta * theta + 1.0))
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                arp, arq = a[:, p].copy(), a[:, q].copy()
                a[:, p] = a[p, :] = c * arp - s * arq
                a[:, q] = a[q, :] = s * arp + c * arq
                a[p, p], a[q, q] = arp[p] - t * apq, arq[q] + t * apq
                a[p, q] = a[q, p] = 0.0
                vp, vq = v[:, p].copy(), v[:, q].copy()
                v[:, p], v[:, q] = c * vp - s * vq, s * vp + c * vq
    return np.diag(a).copy(), v


def pose_from_h(h):
    """h = [M | m] -> (R, t): R = M (M^T M)^(-1/2), t = m / (mean singular value of M); both negated when det M < 0."""
    H = np.asarray(h, dtype=np.float64).reshape(3, 4)
    M, m = H[:, :3].copy(), H[:, 3].copy()
    if np.linalg.det(M) < 0:
        M, m = -M, -m
    lam, W = jacobi_eigh(M.T @ M, SWEEPS3)
    with np.errstate(all="ignore"):
        sig = np.sqrt(lam)
        R = M @ (W @ np.diag(1.0 / sig) @ W.T)
        t = m / (sig.sum() / 3.0)
    return R, t


def linear_pose(X, uv, K):
    """-> dict(R, t, h, eig): the linear stage over the correspondences in order; `eig` the sorted Jacobi eigenvalues."""
    uvn = normalise_pixels(uv, K)
    lam, V = jacobi_eigh(ata_from_sums(forty_sums(np.asarray(X, dtype=np.float64), uvn)), SWEEPS12)
    h = V[:, int(np.argmin(lam))]
    R, t = pose_from_h(h)
    return dict(R=R, t=t, h=h, eig=np.sort(lam))


def params_from_pose(R, t):
    """(R, t) of x_cam = R X + t -> (omega, T = -R^T t), the six parameters of the bundle-adjustment model."""
    return np.concatenate([orc.rotvec_from_matrix(R), -R.T @ t])


def pose_from_params(p):
    """(omega, T) -> (R, t = -R T)."""
    R = orc.rodrigues(np.asarray(p[:3], dtype=np.float64))
    return R, -R @ np.asarray(p[3:], dtype=np.float64)


def _linearise(p, X, uv, K):
    """sum |r|^2, g (6), H (6x6), depths of one camera at p over the correspondences."""
    n = len(X)
    x = np.concatenate([p, np.asarray(X, dtype=np.float64).ravel()])
    with np.errstate(all="ignore"):
        r, Jc, _ = orc.jacobian_blocks(x, 1, n, np.zeros(n, dtype=np.int64), np.arange(n), uv, K)
        depth = (X - p[None, 3:]) @ orc.rodrigues(p[:3])[2]
        g = np.einsum("nki,nk->i", Jc, r)
        H = np.einsum("nki,nkj->ij", Jc, Jc)
    return float((r * r).sum()), g, H, depth


def gauss_newton_step(p, X, uv, K):
    """The undamped Gauss-Newton step at p (what the refinement would take next)."""
    _, g, H, _ = _linearise(np.asarray(p, dtype=np.float64), X, uv, K)
    return -np.linalg.solve(H, g)


def cost(p, X, uv, K):
    return 0.5 * _linearise(np.asarray(p, dtype=np.float64), X, uv, K)[0]


def refine(p, X, uv, K, max_iter=20, xtol=1e-10):
    """Damped Gauss-Newton from p -> (p, sum |r|^2, depths, trial poses): the schedule of triangulate_ref.triangulate."""
    s, g, H, depth = _linearise(p, X, uv, K)
    lam, it = 0.0, 0
    while it < max_iter:
        with np.errstate(all="ignore"):
            try:
                d = -np.linalg.solve(H + lam * np.diag(np.diag(H)), g)
            except np.linalg.LinAlgError:
                d = np.full(6, np.nan)
        if np.sqrt(d @ d) <= xtol * (np.sqrt(p @ p) + xtol):           # the step on offer is below the tolerance already
            break
        st, gt, Ht, dt = _linearise(p + d, X, uv, K)
        it += 1
        if st <= s:
            p, s, g, H, depth = p + d, st, gt, Ht, dt
            lam = 0.1 * lam if lam > 1e-6 else 0.0
            if np.sqrt(d @ d) <= xtol * (np.sqrt(p @ p) + xtol):
                break
        else:
            if -(g @ d + 0.5 * d @ H @ d) <= 1e-12 * 0.5 * s:          # nothing left that the cost's own rounding would show
                break
            lam = 1e-3 if lam == 0.0 else 10.0 * lam
    return p, s, depth, it


def resect_one(X, uv, K, p0=None, start=0, max_iter=20, min_views=6, xtol=1e-10, min_depth=0.0, max_rms_px=np.inf):
    """One camera from its correspondences in order -> dict(status, params, linear, views, iters, rms_err)."""
    X, uv = np.asarray(X, dtype=np.float64).reshape(-1, 3), np.asarray(uv, dtype=np.float64).reshape(-1, 2)
    out = dict(status=FEW_VIEWS, params=None, linear=None, views=len(X), iters=0, rms_err=np.nan)
    if len(X) < max(min_views, 6 if start == 0 else 3):
        return out
    out["status"] = DEGENERATE
    if start == 0:
        lin = linear_pose(X, uv, K)
        with np.errstate(all="ignore"):
            p = params_from_pose(lin["R"], lin["t"])
        if not lin["eig"][1] > 1e-12 * lin["eig"][-1] or not np.all(np.isfinite(p)):
            return out
        out["linear"] = p
    else:
        p = np.asarray(p0, dtype=np.float64).copy()
    if not np.isfinite(_linearise(p, X, uv, K)[0]) or not np.all(np.isfinite(p)):
        return out
    p, s, depth, it = refine(p, X, uv, K, max_iter, xtol)
    out["iters"], out["rms_err"] = it, np.sqrt(s / len(X))
    if not (np.isfinite(out["rms_err"]) and np.all(np.isfinite(p))):
        return out
    if depth.min() <= min_depth:
        out["status"] = BEHIND
    elif out["rms_err"] > max_rms_px:
        out["status"] = HIGH_ERROR
    else:
        out["status"], out["params"] = OK, p
    return out


def camera_slices(camera_indices, point_indices, n_cameras):
    """Per camera, the caller's observation indices in camera-major stored order: the stored order is point-major
    (stable), the camera-major one a stable sort of that by camera."""
    ci, pi = np.asarray(camera_indices).ravel(), np.asarray(point_indices).ravel()
    stored = np.argsort(pi, kind="stable")
    cm = stored[np.argsort(ci[stored], kind="stable")]
    ptr = np.searchsorted(ci[cm], np.arange(n_cameras + 1))
    return [cm[ptr[c]:ptr[c + 1]] for c in range(n_cameras)]


def resect(x, args, select=None, obs_use=None, **options):
    """-> dict(cameras (C, 6), linear (C, 6), status, views, iters, rms_err): what sfmba_resect returns, plus the linear
    stage's parameters (NaN where there are none)."""
    C, P, ci, pi, uv, K = args
    x = np.asarray(x, dtype=np.float64)
    pi, uv = np.asarray(pi).ravel(), np.asarray(uv, dtype=np.float64)
    pts = x[6 * C:].reshape(P, 3)
    use = np.ones(len(pi), dtype=bool) if obs_use is None else np.asarray(obs_use).ravel() != 0
    sel = np.ones(C, dtype=bool) if select is None else np.asarray(select).ravel() != 0
    out = dict(cameras=x[:6 * C].reshape(C, 6).copy(), linear=np.full((C, 6), np.nan),
               status=np.full(C, NOT_SELECTED, dtype=np.int32), views=np.zeros(C, dtype=np.int32),
               iters=np.zeros(C, dtype=np.int32), rms_err=np.full(C, np.nan))
    slices = camera_slices(ci, pi, C)
    for c in np.flatnonzero(sel):
        idx = slices[c][use[slices[c]]]
        r = resect_one(pts[pi[idx]], uv[idx], K, p0=x[6 * c:6 * c + 6], **options)
        out["status"][c], out["views"][c], out["iters"][c], out["rms_err"][c] = r["status"], r["views"], r["iters"], r["rms_err"]
        if r["linear"] is not None:
            out["linear"][c] = r["linear"]
        if r["status"] == OK:
            out["cameras"][c] = r["params"]
    return out


def rotation_angle(Ra, Rb):
    """Angle of Ra^T Rb in radians, as atan2 of the skew part's norm and the trace (safe near 0 and near pi)."""
    D = np.asarray(Ra).T @ np.asarray(Rb)
    sk = 0.5 * np.array([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]])
    return float(np.arctan2(np.sqrt(sk @ sk), 0.5 * (np.trace(D) - 1.0)))
