"""CPU reference of sfmba_covariance (numpy only) and the cases its tests and tools/gen_covariance_golden.py share.

The dense Jacobian comes from oracle.ba_oracle.jacobian_blocks, the held set from the rule of include/sfmba.h, and every
block by two routes that differ in the order of summation: (A) numpy.linalg.inv of the whole reduced J^T J (cameras and
points together), (B) the Schur route with Cholesky factors.  Their spread, times the factor of the bounds file, is what
the GPU is held to.  The error measure of a block is max |a_ij - b_ij| / sqrt(b_ii b_jj), which is scale-free."""
import json
import os

import numpy as np

from oracle import ba_oracle as orc

HERE = os.path.dirname(os.path.abspath(__file__))
BOUNDS_PATH = os.path.join(HERE, "golden", "covariance_bounds.json")
FACTOR = 100.0                 # the factor tests/golden/triangulate_bounds.json uses: summation order and FMA contraction
RANK_TOL, POINT_TOL = 1e-10, 1e-12
FREE, HELD, UNOBSERVED = 0, 1, 2


def held_mask(x, n_cameras, camera_indices, fixed=(), hold=(), gauge=True):
    """(mask (6C,) uint8: 0 free, 1 held, 2 unobserved; (g0, g1, axis)) by the rule of sfmba_covariance."""
    C = int(n_cameras)
    x = np.asarray(x, dtype=np.float64)
    views = np.bincount(np.asarray(camera_indices), minlength=C)
    fixed = sorted(set(int(c) for c in fixed))
    hold = [int(q) for q in hold]
    mask = np.zeros(6 * C, dtype=np.uint8)
    for c in fixed:
        mask[6 * c:6 * c + 6] = HELD
    mask[hold] = HELD
    g = (-1, -1, -1)
    if gauge and not hold and len(fixed) < 2:
        g0 = fixed[0] if fixed else 0
        T = x[:6 * C].reshape(C, 6)[:, 3:]
        d = np.sqrt(((T - T[g0]) ** 2).sum(axis=1))
        g1, best = -1, -1.0
        for c in range(C):
            if c != g0 and views[c] > 0 and d[c] > best:
                g1, best = c, d[c]
        axis = -1
        mask[6 * g0:6 * g0 + 6] = HELD
        if g1 >= 0:
            axis = int(np.argmax(np.abs(T[g1] - T[g0])))       # (the first of equal components)
            mask[6 * g1 + 3 + axis] = HELD
        g = (g0, g1, axis)
    for c in range(C):
        if views[c] == 0:
            mask[6 * c:6 * c + 6] = UNOBSERVED
    return mask, g


def block_error(a, b):
    """max |a_ij - b_ij| / sqrt(b_ii b_jj) over the last two axes (square blocks); an entry whose scale is zero (a held
    row or column) must agree exactly."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    d = np.sqrt(np.abs(np.diagonal(b, axis1=-2, axis2=-1)))
    scale = d[..., :, None] * d[..., None, :]
    diff = np.abs(a - b)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(scale > 0, diff / scale, np.where(diff == 0, 0.0, np.inf))
    rel = np.where(np.isnan(a) & np.isnan(b), 0.0, rel)
    return float(np.max(rel)) if rel.size else 0.0


def _chol_pivots(A, tol):
    """Right-looking Cholesky with the relative pivot test d_k > tol A_kk.  -> (L or None, smallest d_k / A_kk, failing k or -1)."""
    A = np.array(A, dtype=np.float64)
    n = A.shape[0]
    d0 = np.diag(A).copy()
    minrel = np.inf
    for k in range(n):
        d = A[k, k]
        if not d > tol * d0[k]:
            return None, minrel, k
        minrel = min(minrel, d / d0[k])
        A[k:, k] /= np.sqrt(d)
        A[k + 1:, k + 1:] -= np.outer(A[k + 1:, k], A[k + 1:, k])
    return np.tril(A), minrel, -1


def linearise(x, args):
    """r (N,2), Jc (N,2,6), Jp (N,2,3) and the blocks U (C,6,6), V (P,3,3), W per observation (N,6,3)."""
    C, P, ci, pi = int(args[0]), int(args[1]), np.asarray(args[2]), np.asarray(args[3])
    r, Jc, Jp = orc.jacobian_blocks(np.asarray(x, dtype=np.float64), *args)
    U = np.zeros((C, 6, 6))
    V = np.zeros((P, 3, 3))
    np.add.at(U, ci, np.einsum("nku,nkv->nuv", Jc, Jc))
    np.add.at(V, pi, np.einsum("nku,nkv->nuv", Jp, Jp))
    W = np.einsum("nku,nkv->nuv", Jc, Jp)
    return r, Jc, Jp, U, V, W


def reduced_camera_matrix(x, args, mask=None):
    """S = U - sum W V^-1 W^T (6C, 6C) at x over the points with observations; rows and columns with mask != 0 replaced by
    identity (mask None: nothing held)."""
    C, P, ci, pi = int(args[0]), int(args[1]), np.asarray(args[2]), np.asarray(args[3])
    _, _, _, U, V, W = linearise(x, args)
    S = np.zeros((6 * C, 6 * C))
    for c in range(C):
        S[6 * c:6 * c + 6, 6 * c:6 * c + 6] = U[c]
    for p in np.unique(pi):
        obs = np.nonzero(pi == p)[0]
        Wp = np.zeros((6 * C, 3))
        for k in obs:
            Wp[6 * ci[k]:6 * ci[k] + 6] += W[k]
        S -= Wp @ np.linalg.inv(V[p]) @ Wp.T
    if mask is not None:
        h = np.asarray(mask) != 0
        S[h, :] = 0.0
        S[:, h] = 0.0
        S[h, h] = 1.0
    return S


def covariance(x, args, fixed=(), hold=(), gauge=True, kind=0, sigma2=None, route="B", rank_tol=RANK_TOL, point_tol=POINT_TOL):
    """The quantities of sfmba_covariance by route "A" (inverse of the whole reduced J^T J) or "B" (Schur + Cholesky)."""
    C, P, ci, pi = int(args[0]), int(args[1]), np.asarray(args[2]), np.asarray(args[3])
    N = len(ci)
    x = np.asarray(x, dtype=np.float64)
    r, Jc, Jp, U, V, W = linearise(x, args)
    mask, g = held_mask(x, C, ci, fixed, hold, gauge)
    free = mask == FREE
    pt_views = np.bincount(pi, minlength=P)
    n_obs_pts = int((pt_views > 0).sum())
    dof = 2 * N - int(free.sum()) - 3 * n_obs_pts
    sum_r2 = float((r ** 2).sum())
    out = {"held": mask, "gauge": g, "dof": dof, "cost": 0.5 * sum_r2, "status": 0, "bad_param": -1, "n_free": int(free.sum()),
           "n_held": int((mask == HELD).sum())}
    s2 = float(sigma2) if sigma2 else (sum_r2 / dof if dof > 0 else 1.0)
    out["sigma2"] = s2
    # points: pivots of the 3x3 Cholesky
    pt_status = np.where(pt_views > 0, 0, 3).astype(np.int32)
    pt_piv = np.full(P, np.inf)
    Vinv = np.zeros((P, 3, 3))
    for p in range(P):
        if pt_views[p] == 0:
            continue
        L, _, bad = _chol_pivots(V[p], 0.0)                                # the pivots are d_k = L_kk^2
        if bad >= 0 or not np.min(np.diag(L) ** 2) > point_tol * np.max(np.diag(V[p])):
            pt_status[p] = 1
            continue
        pt_piv[p] = np.min(np.diag(L) ** 2) / np.max(np.diag(V[p]))
        Li = np.linalg.inv(L)
        Vinv[p] = Li.T @ Li if route == "B" else np.linalg.inv(V[p])
    out["pt_status"] = pt_status
    out["pt_min_pivot"] = float(np.min(pt_piv[pt_status == 0])) if (pt_status == 0).any() else np.inf
    nan6 = np.full((C, 6, 6), np.nan)
    nanp = np.full((P, 3, 3), np.nan)
    if (pt_status == 1).any():
        out.update(status=2, n_bad_points=int((pt_status == 1).sum()), bad_point=int(np.nonzero(pt_status == 1)[0][0]),
                   cam_cov=nan6, cam_full=np.full((6 * C, 6 * C), np.nan), pt_cov=nanp)
        return out
    fidx = np.nonzero(free)[0]
    unobs = mask == UNOBSERVED
    pt_cov = nanp.copy()
    if kind == 1:
        full = np.zeros((6 * C, 6 * C))
        minrel = np.inf
        for c in range(C):
            f = np.nonzero(free[6 * c:6 * c + 6])[0]
            if len(f) == 0:
                continue
            Uf = U[c][np.ix_(f, f)]
            L, mr, bad = _chol_pivots(Uf, rank_tol)
            minrel = min(minrel, mr)
            if bad >= 0:
                out.update(status=1, bad_param=6 * c + int(f[bad]), cam_cov=nan6, cam_full=np.full((6 * C, 6 * C), np.nan),
                           pt_cov=nanp)
                return out
            if route == "B":
                Li = np.linalg.inv(L)
                inv = Li.T @ Li
            else:
                inv = np.linalg.inv(Uf)
            full[np.ix_(6 * c + f, 6 * c + f)] = s2 * inv
        out["min_pivot_rel"] = minrel
        ok = pt_status == 0
        pt_cov[ok] = s2 * Vinv[ok]
    elif route == "B":
        S = np.zeros((6 * C, 6 * C))
        for c in range(C):
            S[6 * c:6 * c + 6, 6 * c:6 * c + 6] = U[c]
        Y = np.einsum("nuv,nvw->nuw", W, Vinv[pi])                      # W_a V^-1, per observation
        WY = {}
        for k in range(N):                                                 # sum over the pairs of observations of a point
            WY.setdefault(int(pi[k]), []).append(k)
        for p, obs in WY.items():
            for a in obs:
                for b in obs:
                    S[6 * ci[a]:6 * ci[a] + 6, 6 * ci[b]:6 * ci[b] + 6] -= Y[a] @ W[b].T
        S = 0.5 * (S + S.T)
        Sf = S[np.ix_(fidx, fidx)]
        L, minrel, bad = _chol_pivots(Sf, rank_tol)
        out["min_pivot_rel"] = minrel
        if bad >= 0:
            out.update(status=1, bad_param=int(fidx[bad]), cam_cov=nan6, cam_full=np.full((6 * C, 6 * C), np.nan), pt_cov=nanp)
            return out
        Li = np.linalg.inv(L)
        full = np.zeros((6 * C, 6 * C))
        full[np.ix_(fidx, fidx)] = s2 * (Li.T @ Li)
        for p, obs in WY.items():
            acc = s2 * Vinv[p]
            for a in obs:
                Z = np.zeros((6, 3))
                for b in obs:
                    Z += full[6 * ci[a]:6 * ci[a] + 6, 6 * ci[b]:6 * ci[b] + 6] @ Y[b]
                acc = acc + Y[a].T @ Z
            pt_cov[p] = acc
    else:
        # the whole reduced normal matrix: free camera parameters | the parameters of the observed points
        pts_on = np.nonzero(pt_views > 0)[0]
        col_of_pt = -np.ones(P, dtype=np.int64)
        col_of_pt[pts_on] = np.arange(len(pts_on))
        col_of_cam = -np.ones(6 * C, dtype=np.int64)
        col_of_cam[fidx] = np.arange(len(fidx))
        nf = len(fidx)
        J = np.zeros((2 * N, nf + 3 * len(pts_on)))
        for k in range(N):
            for u in range(6):
                q = col_of_cam[6 * ci[k] + u]
                if q >= 0:
                    J[2 * k:2 * k + 2, q] += Jc[k][:, u]
            q = nf + 3 * col_of_pt[pi[k]]
            J[2 * k:2 * k + 2, q:q + 3] = Jp[k]
        Hinv = np.linalg.inv(J.T @ J)
        out["min_pivot_rel"] = np.nan
        full = np.zeros((6 * C, 6 * C))
        full[np.ix_(fidx, fidx)] = s2 * Hinv[:nf, :nf]
        for p in pts_on:
            q = nf + 3 * col_of_pt[p]
            pt_cov[p] = s2 * Hinv[q:q + 3, q:q + 3]
    full[unobs, :] = np.nan
    full[:, unobs] = np.nan
    out["cam_full"] = full
    out["cam_cov"] = np.stack([full[6 * c:6 * c + 6, 6 * c:6 * c + 6] for c in range(C)])
    out["pt_cov"] = pt_cov
    return out


# ---- the cases ---------------------------------------------------------------------------------------------------------------
def _pb(C, P, N, seed):
    import sfmba
    return sfmba.make_problem(C, P, N, seed=seed)


def _single_camera_points(pb):
    """Points all of whose observations come from one camera: undetermined along the ray."""
    return [int(p) for p in np.unique(pb.point_indices)
            if len(np.unique(pb.camera_indices[pb.point_indices == p])) < 2]


def _case_c3(fixed=(), drop=True):
    import sfmba
    pb = _pb(3, 40, 240, 1)
    if drop:
        pb = sfmba.drop_observations(pb, points=(2, 4, 16))
    return dict(x=pb.x_true, args=pb.args, fixed=tuple(fixed))


def _case_c11(dup=False, gauge=True):
    pb = _pb(11, 200, 1600, 2)
    args = pb.args
    if dup:                                       # observation 100 once more, right behind itself: its camera sees the point twice
        k = 100
        ci, pi, uv = (np.insert(a, k + 1, a[k], axis=0) for a in (pb.camera_indices, pb.point_indices, pb.points_2d))
        args = (pb.n_cameras, pb.n_points, ci, pi, uv, pb.K)
    return dict(x=pb.x_true, args=args, gauge=gauge)


def _case_c21():
    pb = _pb(21, 300, 3000, 3)
    return dict(x=pb.x_true, args=pb.args)


def _case_grid21():
    """Every one of the 21 cameras of make_problem(21, 12, 252, seed=5) observes every one of its 12 points; pixels are
    re-projected from x_true with 0.5 px noise, seed 0: every track has 21 views."""
    pb = _pb(21, 12, 252, 5)
    C, P = 21, 12
    pi = np.repeat(np.arange(P, dtype=np.int64), C)
    ci = np.tile(np.arange(C, dtype=np.int64), P)
    zero = np.zeros((C * P, 2))
    r = orc.compute_residuals_loop(pb.x_true, C, P, ci, pi, zero, pb.K).reshape(-1, 2)
    uv = r + np.random.default_rng(0).normal(0.0, 0.5, r.shape)
    return dict(x=pb.x_true, args=(C, P, ci, pi, uv, pb.K))


def _case_grid21_multi():
    """The same 21 cameras and the first six points, seen 1, 1, 2, 2, 32 / 21 and 4 times by every camera: runs of 21, 21, 42,
    42, 32 and 84 observations -- below, at and above the switch-over of the point sweep's lane / wave split (32), and more
    than one block of 64 -- with a pixel of its own (0.5 px noise, seed 1) for every observation."""
    pb = _pb(21, 12, 252, 5)
    C, P = 21, 6
    cams = np.arange(C, dtype=np.int64)
    runs = [cams, cams, np.repeat(cams, 2), np.tile(cams, 2), np.concatenate([cams, cams[:11]]), np.tile(cams, 4)]
    ci = np.concatenate(runs)
    pi = np.concatenate([np.full(len(r), p, dtype=np.int64) for p, r in enumerate(runs)])
    x = np.concatenate([pb.x_true[:6 * C], pb.x_true[6 * C:6 * C + 3 * P]])
    r = orc.compute_residuals_loop(x, C, P, ci, pi, np.zeros((len(ci), 2)), pb.K).reshape(-1, 2)
    uv = r + np.random.default_rng(1).normal(0.0, 0.5, r.shape)
    return dict(x=x, args=(C, P, ci, pi, uv, pb.K))


def _case_cond40():
    import sfmba
    pb = _pb(40, 300, 2000, 4)
    pb = sfmba.drop_observations(pb, points=_single_camera_points(pb))
    return dict(x=pb.x_true, args=pb.args, kind=1)


CASES = {
    "c3": lambda: _case_c3(),
    "c3_fixed0": lambda: _case_c3(fixed=(0,)),
    "c3_fixed01": lambda: _case_c3(fixed=(0, 1)),
    "c11": lambda: _case_c11(),
    "c11_dup": lambda: _case_c11(dup=True),
    "c21": lambda: _case_c21(),
    "grid21": lambda: _case_grid21(),
    "grid21_multi": lambda: _case_grid21_multi(),
    "cond40": lambda: _case_cond40(),
}
FAILING = {                                      # no bounds: the call reports a rank failure
    "c3_undropped": lambda: _case_c3(drop=False),
    "c11_nogauge": lambda: _case_c11(gauge=False),
}
_made = {}


def case(name):
    """The arguments of a case (built once): x, args, and fixed / hold / gauge / kind where they differ from the defaults."""
    if name not in _made:
        d = dict(fixed=(), hold=(), gauge=True, kind=0)
        d.update((CASES.get(name) or FAILING[name])())
        _made[name] = d
    return _made[name]


def case_bounds(name):
    """What tools/gen_covariance_golden.py records of a case: the spread of the two routes per kind of block, the smallest
    relative pivots, and the spectrum of the unheld S (marginal cases)."""
    c = case(name)
    kw = dict(fixed=c["fixed"], hold=c["hold"], gauge=c["gauge"], kind=c["kind"])
    A, B = covariance(c["x"], c["args"], route="A", **kw), covariance(c["x"], c["args"], route="B", **kw)
    assert A["status"] == 0 and B["status"] == 0, name
    ok = B["pt_status"] == 0
    rec = {
        "spread_cam": max(block_error(A["cam_full"], B["cam_full"]), block_error(B["cam_full"], A["cam_full"])),
        "spread_cam_cov": max(block_error(A["cam_cov"], B["cam_cov"]), block_error(B["cam_cov"], A["cam_cov"])),
        "spread_pt": max(block_error(A["pt_cov"][ok], B["pt_cov"][ok]), block_error(B["pt_cov"][ok], A["pt_cov"][ok])),
        "min_pivot_rel": float(B["min_pivot_rel"]),
        "pt_min_pivot": float(B["pt_min_pivot"]),
        "dof": int(B["dof"]),
        "gauge": [int(v) for v in B["gauge"]],
    }
    if c["kind"] == 0:
        ev = np.sort(np.abs(np.linalg.eigvalsh(reduced_camera_matrix(c["x"], c["args"], np.asarray(B["held"]) == UNOBSERVED))))
        n_fixed = 6 * len(c["fixed"])           # a held camera's rows are identity in the pair lists' S too: not counted
        rec["null_eig_rel"] = float(ev[6] / ev[-1]) if n_fixed == 0 else None
        rec["eighth_eig_rel"] = float(ev[7] / ev[-1]) if n_fixed == 0 else None
    return rec


def accept(name, rec, rank_tol=RANK_TOL, point_tol=POINT_TOL):
    """The conditions under which a case may serve: its pivots are far from the tolerances, and (nothing held by the
    problem) the unheld S shows seven eigenvalues below rank_tol of the largest."""
    if not rec["min_pivot_rel"] > 100.0 * rank_tol:
        return "smallest gauged pivot %.3g within 100x of rank_tol" % rec["min_pivot_rel"]
    if not rec["pt_min_pivot"] > 100.0 * point_tol:
        return "smallest point pivot %.3g within 100x of point_tol" % rec["pt_min_pivot"]
    if rec.get("null_eig_rel") is not None and not (rec["null_eig_rel"] < rank_tol and rec["eighth_eig_rel"] > rank_tol):
        return "the unheld S does not show seven null eigenvalues (%.3g, %.3g)" % (rec["null_eig_rel"], rec["eighth_eig_rel"])
    return None


def load_bounds():
    with open(BOUNDS_PATH) as f:
        return json.load(f)
