"""numpy restatement of sfmba_resect_ransac (include/sfmba.h): the counter-based draw of three positions, Grunert's P3P
with the quartic's real roots in closed form (Ferrari through the largest root of the resolvent cubic, then two Newton
steps), the pose by aligning the two triangles, the score of every solution, the best hypothesis, its mask and the
refinement over the inliers (resect_ref.refine).  Written for the tests: plain loops, one camera at a time.

Beside its result a hypothesis carries the flag `close`: a decision inside it was within CLOSE (relative) of going the
other way, so a second implementation in other rounding may legitimately count differently.  The tests compare counts
only where the flag is down.  The flag is raised by a decision of the solver (root separation, a discriminant's sign,
|cg - v ca|, v or u against 0) within CLOSE, relative, of flipping, and by a scored squared error of ANY of the hypothesis'
solutions within 1e-6 threshold^2 of the threshold.  Two solutions that merely tie in count raise no flag: with equal
counts both implementations keep the lower solution, and a count that could differ is what the second trigger catches (at
n = 8 most hypotheses hold two solutions that count their own three points and nothing else)."""
import numpy as np

import resect_ref as rr

NOT_SELECTED, OK, FEW_VIEWS, DEGENERATE, BEHIND, HIGH_ERROR = -1, 0, 1, 2, 3, 4
CLOSE = 1e-4
COLLINEAR = 1e-9                                                 # sine of the angle at P1 below which a triple counts as collinear
M64 = (1 << 64) - 1
GOLD = 0x9e3779b97f4a7c15


def mix(z):
    z &= M64
    z ^= z >> 30; z = (z * 0xbf58476d1ce4e5b9) & M64
    z ^= z >> 27; z = (z * 0x94d049bb133111eb) & M64
    z ^= z >> 31
    return z


def draw3(seed, c, h, n):
    """Three distinct positions among n >= 3: a function of (seed, camera index in the problem, h) alone."""
    key = mix(int(seed) ^ mix((int(c) << 32) | int(h)))
    out, srt = [], []
    for j in range(3):
        k = mix(key + (j + 1) * GOLD) % (n - j)
        for s in srt:                                            # the earlier choices, ascending
            if k >= s:
                k += 1
        out.append(int(k))
        srt = sorted(srt + [int(k)])
    return out


def draw_samples(seed, c, H, n):
    return np.array([draw3(seed, c, h, n) for h in range(H)], dtype=np.int32).reshape(H, 3)


def _near(value, scale):
    return abs(value) <= CLOSE * abs(scale)


def quartic_real_roots(A):
    """Real roots of A[4] v^4 + ... + A[0], ascending, after two Newton steps -> (roots, close).  A NaN or infinite
    coefficient gives none."""
    close = False
    with np.errstate(all="ignore"):
        b, c, d, e = A[3] / A[4], A[2] / A[4], A[1] / A[4], A[0] / A[4]
        if not np.isfinite(b + c + d + e):
            return [], True
        if _near(A[4], max(abs(x) for x in A)):
            close = True
        # depressed quartic y^4 + p y^2 + q y + r, v = y - b / 4
        p = c - 0.375 * b * b
        q = d - 0.5 * b * c + 0.125 * b * b * b
        r = e - 0.25 * b * d + 0.0625 * b * b * c - (3.0 / 256.0) * b * b * b * b
        # resolvent cubic z^3 + 2 p z^2 + (p^2 - 4 r) z - q^2 = 0: its largest real root (never negative)
        B, Cc, D = 2.0 * p, p * p - 4.0 * r, -q * q
        P3 = Cc - B * B / 3.0
        Q3 = 2.0 * B * B * B / 27.0 - B * Cc / 3.0 + D
        disc = 0.25 * Q3 * Q3 + P3 * P3 * P3 / 27.0
        if _near(disc, 0.25 * Q3 * Q3 + abs(P3 * P3 * P3) / 27.0):
            close = True
        if disc > 0.0:
            sq = np.sqrt(disc)
            w = np.cbrt(-0.5 * Q3 + sq) + np.cbrt(-0.5 * Q3 - sq)
        else:
            m = np.sqrt(-P3 / 3.0)
            arg = 3.0 * Q3 / (2.0 * P3 * m) if m > 0.0 else 0.0
            arg = min(1.0, max(-1.0, arg))
            w = 2.0 * m * np.cos(np.arccos(arg) / 3.0)
        z = w - B / 3.0
        if abs(z) <= CLOSE * CLOSE * (abs(w) + abs(B / 3.0)):    # (z >= 0 in exact arithmetic: only its cancellation can flip the test)
            close = True
        if not z > 0.0:
            return [], True
        s = np.sqrt(z)
        t = 0.5 * (p + z - q / s)
        u = 0.5 * (p + z + q / s)
        roots = []
        for sgn, tt in ((-1.0, t), (1.0, u)):                    # y^2 + s y + t, then y^2 - s y + u
            dq = z - 4.0 * tt
            if _near(dq, abs(z) + 4.0 * abs(tt)):
                close = True
            if dq >= 0.0:
                rt = np.sqrt(dq)
                roots += [0.5 * (sgn * s - rt) - 0.25 * b, 0.5 * (sgn * s + rt) - 0.25 * b]
        out = []
        for v in roots:
            for _ in range(2):
                f = (((v + b) * v + c) * v + d) * v + e
                fp = ((4.0 * v + 3.0 * b) * v + 2.0 * c) * v + d
                v = v - f / fp
            out.append(v)
    out = sorted(out, key=lambda x: (not np.isfinite(x), x))
    for i in range(len(out) - 1):
        if not np.isfinite(out[i] + out[i + 1]) or _near(out[i + 1] - out[i], max(abs(out[i]), abs(out[i + 1]))):
            close = True
    return out, close


def _frame(A1, A2, A3):
    with np.errstate(all="ignore"):
        e1 = (A2 - A1) / np.linalg.norm(A2 - A1)
        e3 = np.cross(e1, A3 - A1)
        e3 = e3 / np.linalg.norm(e3)
        e2 = np.cross(e3, e1)
        sine = np.linalg.norm(np.cross(e1, A3 - A1)) / np.linalg.norm(A3 - A1)
    return np.stack([e1, e2, e3], axis=1), sine                  # columns; the sine of the angle at A1


def p3p(P, uv, K):
    """P (3, 3) points, uv (3, 2) pixels -> (solutions [(R, T)] with x_cam = R (X - T), at most four, ascending in
    v = s3 / s1; close)."""
    P, uv = np.asarray(P, dtype=np.float64), np.asarray(uv, dtype=np.float64)
    Kinv = np.linalg.inv(np.asarray(K, dtype=np.float64))
    with np.errstate(all="ignore"):
        j = np.concatenate([uv, np.ones((3, 1))], axis=1) @ Kinv.T
        j = j / np.linalg.norm(j, axis=1, keepdims=True)
        ca, cb, cg = j[1] @ j[2], j[0] @ j[2], j[0] @ j[1]
        a2, b2, c2 = ((P[1] - P[2]) ** 2).sum(), ((P[0] - P[2]) ** 2).sum(), ((P[0] - P[1]) ** 2).sum()
        p, q = (a2 - c2) / b2, (a2 + c2) / b2
        A = [(1.0 + p) ** 2 - 4.0 * (a2 / b2) * cg * cg,
             4.0 * (-p * (1.0 + p) * cb + 2.0 * (a2 / b2) * cg * cg * cb - (1.0 - q) * ca * cg),
             2.0 * (p * p - 1.0 + 2.0 * p * p * cb * cb + 2.0 * ((b2 - c2) / b2) * ca * ca - 4.0 * q * ca * cb * cg
                    + 2.0 * ((b2 - a2) / b2) * cg * cg),
             4.0 * (p * (1.0 - p) * cb - (1.0 - q) * ca * cg + 2.0 * (c2 / b2) * ca * ca * cb),
             (p - 1.0) ** 2 - 4.0 * (c2 / b2) * ca * ca]
        if not np.all(np.isfinite(A)):
            return [], False
        roots, close = quartic_real_roots(A)
        EP, sine = _frame(P[0], P[1], P[2])
        if not sine > COLLINEAR:                                 # a collinear (or repeated: NaN) triple has no solution
            return [], _near(sine - COLLINEAR, COLLINEAR)
        if _near(sine - COLLINEAR, COLLINEAR):
            close = True
        sols = []
        for v in roots:
            den = 2.0 * (cg - v * ca)
            u = ((p - 1.0) * v * v - 2.0 * p * cb * v + 1.0 + p) / den
            if _near(den, 2.0 * (abs(cg) + abs(v * ca))) or _near(v, 1.0) or _near(u, 1.0):
                close = True
            if not (v > 0.0 and u > 0.0 and np.isfinite(u) and np.isfinite(v)):
                continue
            s1 = np.sqrt(b2 / (1.0 + v * v - 2.0 * v * cb))
            Q = np.stack([s1 * j[0], u * s1 * j[1], v * s1 * j[2]])
            R = _frame(Q[0], Q[1], Q[2])[0] @ EP.T
            T = P[0] - R.T @ Q[0]
            if np.all(np.isfinite(R)) and np.all(np.isfinite(T)):
                sols.append((R, T))
    return sols, close


def exact_samples(seed, count, K):
    """`count` valid exact samples: a random pose (rotation up to ~1 rad), three points 4..9 units in front of it and
    their exact pixels -> yields (X (3, 3), uv (3, 2), rotation vector, centre)."""
    rng = np.random.default_rng(seed)
    K = np.asarray(K, dtype=np.float64)
    for _ in range(count):
        w = rng.normal(size=3)
        w *= rng.uniform(0.2, 1.0) / np.linalg.norm(w)
        T = rng.normal(0.0, 1.5, 3)
        cam = np.stack([rng.uniform(-1.8, 1.8, 3), rng.uniform(-1.3, 1.3, 3), rng.uniform(4.0, 9.0, 3)], axis=1)
        uv = cam @ K.T
        yield cam @ rr.orc.rodrigues(w) + T, uv[:, :2] / uv[:, 2:3], w, T


def errors2(R, T, X, uv, K):
    """Squared reprojection error and depth of every correspondence at x_cam = R (X - T)."""
    with np.errstate(all="ignore"):
        q = (np.asarray(X) - T) @ R.T
        pix = q @ np.asarray(K).T
        d = pix[:, :2] / pix[:, 2:3] - uv
    return (d * d).sum(axis=1), q[:, 2]


def inliers(R, T, X, uv, K, threshold, min_depth):
    e2, depth = errors2(R, T, X, uv, K)
    with np.errstate(invalid="ignore"):
        return (e2 < threshold * threshold) & (depth > min_depth) & np.isfinite(e2), e2


def hypothesis(X, uv, K, idx, threshold, min_depth):
    """-> dict(count, sol, R, T, mask, close, n_sol): the score of the sample idx (three positions); count -1 for a sample
    with a repeated position, 0 and sol -1 when there is no solution."""
    if len(set(int(i) for i in idx)) < 3:
        return dict(count=-1, sol=-1, R=None, T=None, mask=None, close=False, n_sol=0)
    sols, close = p3p(X[list(idx)], uv[list(idx)], K)
    best = dict(count=0, sol=-1, R=None, T=None, mask=None, close=close, n_sol=len(sols))
    t2 = threshold * threshold
    for s, (R, T) in enumerate(sols):
        m, e2 = inliers(R, T, X, uv, K, threshold, min_depth)
        # a scored error at the threshold: this solution's count may differ by one elsewhere, and with it the winner
        if np.any(np.abs(e2 - t2) <= 1e-6 * t2):
            best["close"] = True
        if best["sol"] < 0 or int(m.sum()) > best["count"]:
            best.update(count=int(m.sum()), sol=s, R=R, T=T, mask=m)
    return best


def ransac_one(X, uv, K, c=0, samples=None, seed=0, max_iters=256, threshold=8.0, confidence=0.99, min_depth=0.0,
               min_views=6, refine=1, max_iter=20, xtol=1e-10, max_rms_px=np.inf):
    """One camera from its used correspondences in order -> dict(status, params, hyp, mask, views, inliers, best,
    best_sol, success, iters, rms_err, hyp_inliers, hyp_close)."""
    X, uv = np.asarray(X, dtype=np.float64).reshape(-1, 3), np.asarray(uv, dtype=np.float64).reshape(-1, 2)
    n, H = len(X), int(max_iters)
    need = max(int(min_views), 4)
    out = dict(status=FEW_VIEWS, params=None, hyp=None, mask=np.zeros(n, dtype=bool), views=n, inliers=0, best=-1,
               best_sol=-1, success=False, iters=0, rms_err=np.nan, hyp_inliers=np.full(H, -1, dtype=np.int32),
               hyp_close=np.zeros(H, dtype=bool))
    if n < need:
        return out
    if samples is None:
        samples = draw_samples(seed, c, H, n)
    best = None
    for h in range(H):
        r = hypothesis(X, uv, K, samples[h], threshold, min_depth)
        out["hyp_inliers"][h], out["hyp_close"][h] = r["count"], r["close"]
        if best is None or r["count"] > best["count"]:
            best = dict(r, h=h)
    out["status"] = DEGENERATE
    if best["count"] < 0:
        return out
    out["best"], out["best_sol"] = best["h"], best["sol"]
    if best["sol"] < 0:
        return out
    out["mask"], out["inliers"] = best["mask"], best["count"]
    out["success"] = best["count"] / n >= confidence
    out["hyp"] = np.concatenate([rr.orc.rotvec_from_matrix(best["R"]), best["T"]])
    if best["count"] < need:
        return out
    Xi, uvi = X[best["mask"]], uv[best["mask"]]
    p, s, depth, it = rr.refine(out["hyp"].copy(), Xi, uvi, K, max_iter if refine else 0, xtol)
    out["iters"], out["rms_err"] = it, np.sqrt(s / len(Xi))
    if not (np.isfinite(out["rms_err"]) and np.all(np.isfinite(p))):
        return out
    if depth.min() <= min_depth:
        out["status"] = BEHIND
    elif out["rms_err"] > max_rms_px:
        out["status"] = HIGH_ERROR
    else:
        out["status"], out["params"] = OK, p
    return out


def resect_ransac(x, args, select=None, obs_use=None, samples=None, **options):
    """-> dict(cameras, hyp (C, 6), inlier_mask (N, caller's order), status, views, inliers, best, best_sol, success,
    iters, rms_err, hyp_inliers (C, H), hyp_close (C, H)): what sfmba_resect_ransac returns plus the `close` flags."""
    C, P, ci, pi, uv, K = args
    x = np.asarray(x, dtype=np.float64)
    pi, uv = np.asarray(pi).ravel(), np.asarray(uv, dtype=np.float64)
    pts = x[6 * C:].reshape(P, 3)
    use = np.ones(len(pi), dtype=bool) if obs_use is None else np.asarray(obs_use).ravel() != 0
    sel = np.ones(C, dtype=bool) if select is None else np.asarray(select).ravel() != 0
    H = int(options.get("max_iters", 256 if samples is None else np.asarray(samples).shape[1]))
    options["max_iters"] = H
    cams = x[:6 * C].reshape(C, 6).copy()
    out = dict(cameras=cams, hyp=cams.copy(), inlier_mask=np.zeros(len(pi), dtype=bool),
               status=np.full(C, NOT_SELECTED, dtype=np.int32), views=np.zeros(C, dtype=np.int32),
               inliers=np.zeros(C, dtype=np.int32), best=np.full(C, -1, dtype=np.int32),
               best_sol=np.full(C, -1, dtype=np.int32), success=np.zeros(C, dtype=bool), iters=np.zeros(C, dtype=np.int32),
               rms_err=np.full(C, np.nan), hyp_inliers=np.full((C, H), -1, dtype=np.int32),
               hyp_close=np.zeros((C, H), dtype=bool))
    slices = rr.camera_slices(args[2], pi, C)
    for c in np.flatnonzero(sel):
        idx = slices[c][use[slices[c]]]
        r = ransac_one(pts[pi[idx]], uv[idx], K, c=c, samples=None if samples is None else np.asarray(samples)[c], **options)
        for key in ("status", "views", "inliers", "best", "best_sol", "success", "iters", "rms_err", "hyp_inliers", "hyp_close"):
            out[key][c] = r[key]
        out["inlier_mask"][idx] = r["mask"]
        if r["hyp"] is not None:
            out["hyp"][c] = r["hyp"]
        if r["status"] == OK:
            out["cameras"][c] = r["params"]
    return out
