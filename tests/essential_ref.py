"""numpy restatement of the essential-matrix call (include/sfmba.h: sfmba_essential_ransac), written from the header: the
five-point estimate by two routes to the null space (LAPACK's symmetric eigensolver on A^T A, and the SVD of A), the ten
constraints as trilinear forms by einsum, LAPACK's solve where the kernel runs Gauss-Jordan, and companion-matrix
eigenvalues (np.roots) where the kernel brackets roots.  The four null vectors belong to one eigenvalue, zero, so each
route returns its own basis of the same space: candidates agree between routes (and with the device) as matrices up to
sign, not in z or in their order.  There is no reference code for E; the GPU tests compare the device with this file."""
import itertools

import numpy as np

import two_view_ref as tv
from two_view_ref import MASK64, make_pairs, mix

OK, FEW_PAIRS, DEGENERATE = 0, 1, 2
RANK_TOL = 1e-12

# Nister's order  x^3 y^3 x^2y xy^2 x^2z x^2 y^2z y^2 xyz xy | xz^2 xz x yz^2 yz y z^3 z^2 z 1  (x y z 1 = 0 1 2 3)
MONOMIALS = ((0, 0, 0), (1, 1, 1), (0, 0, 1), (0, 1, 1), (0, 0, 2), (0, 0, 3), (1, 1, 2), (1, 1, 3), (0, 1, 2), (0, 1, 3),
             (0, 2, 2), (0, 2, 3), (0, 3, 3), (1, 2, 2), (1, 2, 3), (1, 3, 3), (2, 2, 2), (2, 2, 3), (2, 3, 3), (3, 3, 3))
_ORDERS = [sorted(set(itertools.permutations(m))) for m in MONOMIALS]
_EPS = np.zeros((3, 3, 3))
for _i, _j, _k in itertools.permutations(range(3)):
    _EPS[_i, _j, _k] = np.linalg.det(np.eye(3)[[_i, _j, _k]])


# ---- the sample rule -------------------------------------------------------------------------------------------------
def draw_sample5(seed, e, h, n):
    """The five distinct positions among n >= 5 used pairs of hypothesis h of the batch's edge e."""
    seed, e, h, n = int(seed), int(e), int(h), int(n)
    key = mix(seed ^ mix((e << 32) | h))
    chosen = []
    for j in range(5):
        k = mix((key + (j + 1) * 0x9e3779b97f4a7c15) & MASK64) % (n - j)
        for c in sorted(chosen):
            if k >= c:
                k += 1
        chosen.append(k)
    return chosen


def draw_samples5(seed, e, H, n):
    return np.array([draw_sample5(seed, e, h, n) for h in range(H)], dtype=np.int32).reshape(H, 5)


# ---- the estimate ----------------------------------------------------------------------------------------------------
def to_camera(K, pts):
    q = np.column_stack([pts, np.ones(len(pts))]) @ np.linalg.inv(K).T
    return q[:, :2] / q[:, 2:3]


def null_basis(A, route):
    """X Y Z W (4, 3, 3) of the 5 x 9 matrix A: "eigh" the eigenvectors of the four smallest eigenvalues of A^T A,
    ascending; "svd" the four last right singular vectors of A, from the last."""
    if route == "eigh":
        return np.linalg.eigh(A.T @ A)[1][:, :4].T.reshape(4, 3, 3)
    return np.linalg.svd(A)[2][::-1][:4].reshape(4, 3, 3)


def constraints(B):
    """The 10 x 20 matrix of det E = 0 and 2 E E^T E - tr(E E^T) E = 0 for E = x B0 + y B1 + z B2 + B3."""
    D = np.einsum("ijk,ai,bj,ck->abc", _EPS, B[:, 0], B[:, 1], B[:, 2])
    T = 2.0 * np.einsum("aik,blk,clj->abcij", B, B, B) - np.einsum("akl,bkl,cij->abcij", B, B, B)
    M = np.zeros((10, 20))
    for m, orders in enumerate(_ORDERS):
        for o in orders:
            M[0, m] += D[o]
            M[1:, m] += T[o].ravel()
    return M


def candidates(p1, p2, K, route="eigh"):
    """The candidates of five pixel pairs -> (E (k, 3, 3) by ascending z, z (k)); k = 0 when nothing is finite."""
    c1, c2 = to_camera(K, p1), to_camera(K, p2)
    A = tv.matrix_A(c1, c2)
    none = np.zeros((0, 3, 3)), np.zeros(0)
    if not np.isfinite(A).all():
        return none
    lam = np.linalg.eigvalsh(A.T @ A) if route == "eigh" else np.linalg.svd(A, compute_uv=False)[::-1] ** 2
    if not lam[-5] > RANK_TOL * lam[-1]:                         # the rows have no rank 5 (collinear points): no candidate
        return none
    B = null_basis(A, route)
    M = constraints(B)
    try:
        Rr = np.linalg.solve(M[:, :10], M[:, 10:])
    except np.linalg.LinAlgError:
        return none
    if not np.isfinite(Rr).all():
        return none
    P = np.polynomial.polynomial
    Bz = [[None] * 3 for _ in range(3)]
    for q in range(3):
        ra, rb = Rr[4 + 2 * q], Rr[5 + 2 * q]
        for col, (lo, hi) in enumerate(((0, 3), (3, 6), (6, 10))):
            a, b = ra[lo:hi][::-1], rb[lo:hi][::-1]              # ascending powers of z
            Bz[q][col] = P.polysub(a, P.polymulx(b))
    mul = P.polymul
    p0 = P.polysub(mul(Bz[0][1], Bz[1][2]), mul(Bz[0][2], Bz[1][1]))
    p1_ = P.polysub(mul(Bz[0][2], Bz[1][0]), mul(Bz[0][0], Bz[1][2]))
    p2_ = P.polysub(mul(Bz[0][0], Bz[1][1]), mul(Bz[0][1], Bz[1][0]))
    det = P.polyadd(P.polyadd(mul(p0, Bz[2][0]), mul(p1_, Bz[2][1])), mul(p2_, Bz[2][2]))
    det = np.concatenate([det, np.zeros(11 - len(det))])
    if not np.isfinite(det).all() or not np.any(det[1:] != 0.0):
        return none
    roots = np.roots(np.trim_zeros(det[::-1], "f"))
    zs = np.sort(roots[np.isreal(roots)].real)
    Es = []
    for z in zs:
        b = np.array([[P.polyval(z, Bz[q][col]) for col in range(3)] for q in range(3)])
        crosses = [np.cross(b[0], b[1]), np.cross(b[0], b[2]), np.cross(b[1], b[2])]
        v = crosses[int(np.argmax([c @ c for c in crosses]))]
        with np.errstate(divide="ignore", invalid="ignore"):
            x, y = v[0] / v[2], v[1] / v[2]
            Es.append(x * B[0] + y * B[1] + z * B[2] + B[3])
    return np.array(Es).reshape(-1, 3, 3), zs


def polish(p1, p2, K, E, route="eigh", steps=2):
    """The candidate E of five pixel pairs once more in homogeneous coordinates v (its parts along X Y Z W, unit length):
    `steps` Gauss-Newton steps on the ten cubics with the step kept orthogonal to v, (J^T J + v v^T) d = -J^T c."""
    B = null_basis(tv.matrix_A(to_camera(K, p1), to_camera(K, p2)), route)
    M = constraints(B)
    mono = np.array(MONOMIALS)
    v = np.einsum("kij,ij->k", B, E)
    v = v / np.linalg.norm(v)
    for _ in range(steps):
        c = M @ (v[mono[:, 0]] * v[mono[:, 1]] * v[mono[:, 2]])
        J = np.zeros((10, 4))
        for m, (a, b, cc) in enumerate(MONOMIALS):
            J[:, a] += M[:, m] * v[b] * v[cc]
            J[:, b] += M[:, m] * v[a] * v[cc]
            J[:, cc] += M[:, m] * v[a] * v[b]
        v = v + np.linalg.solve(J.T @ J + np.outer(v, v), -J.T @ c)
        v = v / np.linalg.norm(v)
    out = np.einsum("k,kij->ij", v, B)
    return out if np.isfinite(out).all() else E


def pixel_F(E, K):
    Ki = np.linalg.inv(K)
    return Ki.T @ E @ Ki


def unit_E(E):
    return tv.unit_F(E)


def sign_distance(Ea, Eb):
    """The distance of two matrices as unit-norm matrices up to sign."""
    a, b = Ea / np.linalg.norm(Ea), Eb / np.linalg.norm(Eb)
    return float(min(np.linalg.norm(a - b), np.linalg.norm(a + b)))


def nearest(Es, E):
    """-> (index, distance) of the candidate nearest to E up to sign; (-1, inf) without candidates."""
    if not len(Es):
        return -1, np.inf
    d = [sign_distance(c, E) if np.isfinite(c).all() else np.inf for c in Es]
    return int(np.argmin(d)), float(np.min(d))


def route_distance(p1, p2, K, E_true):
    """The two routes' candidates nearest E_true on one sample -> (their distance from each other, the eigh route's
    distance from E_true, that candidate)."""
    Ea, _ = candidates(p1, p2, K, "eigh")
    Eb, _ = candidates(p1, p2, K, "svd")
    ia, da = nearest(Ea, E_true)
    ib, _ = nearest(Eb, E_true)
    if ia < 0 or ib < 0:
        return np.inf, np.inf, None
    return sign_distance(Ea[ia], Eb[ib]), da, Ea[ia]


def backward_errors(E, K, p1, p2):
    """max |x2^T E x1| over the pairs in camera coordinates, and |2 E E^T E - tr(E E^T) E|_F, of the unit-norm E."""
    E = E / np.linalg.norm(E)
    c1 = np.column_stack([to_camera(K, p1), np.ones(len(p1))])
    c2 = np.column_stack([to_camera(K, p2), np.ones(len(p2))])
    epi = float(np.abs(np.einsum("ni,ij,nj->n", c2, E, c1)).max())
    return epi, float(np.linalg.norm(2.0 * E @ E.T @ E - np.trace(E @ E.T) * E))


def score_hypothesis(Es, K, pts1, pts2, threshold, margin=0.0):
    """-> (count, candidate, near) of a hypothesis: its best candidate's count (the first of equals; 0 and -1 without a
    candidate); near: a candidate that could decide (a count within one of the best) has a pair within margin of the threshold."""
    best, cb, counts, nears = 0, -1, [], []
    for c, E in enumerate(Es):
        d = tv.distances(pixel_F(E, K), pts1, pts2)
        with np.errstate(invalid="ignore"):
            cnt = int(((d < threshold) & np.isfinite(d)).sum())
            nears.append(bool(np.any(np.abs(d - threshold) <= margin)))
        counts.append(cnt)
        if cb < 0 or cnt > best:
            best, cb = cnt, c
    near = any(nr and cnt >= best - 1 for nr, cnt in zip(nears, counts))
    return best, cb, near


def ransac_edge(pts1, pts2, K, samples, threshold=1.0, confidence=0.99, margin=0.0, route="eigh"):
    """One edge over its used pairs with the sample sets `samples` (H, 5) -> dict.  ``near`` (H): see score_hypothesis;
    ``hyp_E`` (H, 3, 3) the best candidate of every hypothesis (zero without one)."""
    n, nh = len(pts1), len(samples)
    out = dict(status=FEW_PAIRS, E=np.zeros((3, 3)), mask=np.zeros(n, dtype=bool), inliers=0, best=-1, success=False,
               hyp=np.full(nh, -1, dtype=np.int32), roots=np.full(nh, -1, dtype=np.int32), near=np.zeros(nh, dtype=bool),
               hyp_E=np.zeros((nh, 3, 3)))
    if n < 5:
        return out
    out["status"] = DEGENERATE
    best = None
    for h, idx in enumerate(np.asarray(samples)):
        if len(set(int(k) for k in idx)) < 5:
            continue
        Es, _ = candidates(pts1[idx], pts2[idx], K, route)
        cnt, cb, near = score_hypothesis(Es, K, pts1, pts2, threshold, margin)
        out["hyp"][h], out["roots"][h], out["near"][h] = cnt, len(Es), near
        if cb >= 0:
            out["hyp_E"][h] = Es[cb]
        if best is None or cnt > out["hyp"][best]:
            best = h
    if best is None:
        return out
    E = out["hyp_E"][best]
    if out["roots"][best] > 0 and np.isfinite(E).all():          # the best candidate is polished; mask and count are the polished one's
        idx = np.asarray(samples)[best]
        E = polish(pts1[idx], pts2[idx], K, E, route)
    mask = tv.inliers(pixel_F(E, K), pts1, pts2, threshold) if out["roots"][best] > 0 else np.zeros(n, dtype=bool)
    out.update(mask=mask, inliers=int(mask.sum()), best=int(best), success=bool(mask.sum() / n >= confidence))
    if out["hyp"][best] < 5 or not np.isfinite(E).all():        # DEGENERATE: count, h and mask are reported, E is not
        return out
    out.update(status=OK, E=unit_E(E))
    return out


def ransac_edge_both(pts1, pts2, K, samples, threshold=1.0, margin=0.0):
    """ransac_edge by the eigh route, and ``skip`` (H): the hypotheses a comparison leaves out -- (a) near the threshold,
    (b) the two routes disagree in the number of real roots or in the count."""
    a = ransac_edge(pts1, pts2, K, samples, threshold, margin=margin, route="eigh")
    b = ransac_edge(pts1, pts2, K, samples, threshold, margin=margin, route="svd")
    a["skip"] = a["near"] | b["near"] | (a["roots"] != b["roots"]) | (a["hyp"] != b["hyp"])
    return a


# ---- synthetic scenes --------------------------------------------------------------------------------------------------
def scene(rng, n, K, kind="general", noise=0.0, outliers=0.0):
    """-> (pts1, pts2, E_true, R, t, is_outlier): "general" a rotation of 0.15 rad and a random baseline, "sideways" R = I
    and t along x (E[2, 2] = 0), over a scene 4..9 units deep."""
    if kind == "sideways":
        p1, p2, R, t, bad = make_pairs(rng, n, K, noise=noise, outliers=outliers, angle=0.0, t_dir=(1.0, 0.0, 0.0))
    else:
        p1, p2, R, t, bad = make_pairs(rng, n, K, noise=noise, outliers=outliers)
    return p1, p2, tv.essential_from_pose(R, t), R, t, bad


# ---- the inputs of tests/test_gpu_essential.py (tests/test_host_essential.py runs the restatement alone on them) ------------
K_TEST = np.array([[800.0, 0.0, 640.0], [0.0, 800.0, 480.0], [0.0, 0.0, 1.0]])
LDS_PAIRS = 4096                                                  # kTwoViewLdsPairs: an edge above it is read from global memory
THRESHOLD, MARGIN = 1.0, 1e-9
# The threshold of the noise-free edges.  A five-point sample has up to ten solutions, and at 1 px a second one fits the three
# other pairs of 12 of the 200 edges as well (count 8 twice; which of the two has the lower z depends on the basis of the
# null space).  At 0.05 px no edge has a second one, and the true candidate's worst distance, 9e-5 px, is 550 times below it.
EXACT_THRESHOLD = 0.05


def batch(edges):
    ptr = np.concatenate([[0], np.cumsum([len(e[0]) for e in edges])]).astype(np.int64)
    return np.concatenate([e[0] for e in edges]), np.concatenate([e[1] for e in edges]), ptr


def count_cases():
    """-> [(name, pts1, pts2, edge_ptr, H, seed of the samples)]: three general edges of 300 pairs with 100 hypotheses, and
    edges at the sizes where the kernel changes its path (below S, S, a wave of lanes, the LDS cap) with 24."""
    rng = np.random.default_rng(2701)
    general = [scene(rng, 300, K_TEST, "general", noise=0.3, outliers=0.25)[:2] for _ in range(3)]
    sizes = [scene(rng, n, K_TEST, "general", noise=0.3, outliers=0.25)[:2] for n in (4, 5, 6, 63, 64, 65, LDS_PAIRS, LDS_PAIRS + 1)]
    return [("general",) + batch(general) + (100, 11), ("sizes",) + batch(sizes) + (24, 12)]


def count_expectation(pts1, pts2, ptr, H, seed):
    """The restatement over a batch with the samples of `seed` -> [per edge: the dict of ransac_edge_both]."""
    out = []
    for e in range(len(ptr) - 1):
        p1, p2 = pts1[ptr[e]:ptr[e + 1]], pts2[ptr[e]:ptr[e + 1]]
        samples = draw_samples5(seed, e, H, len(p1)) if len(p1) >= 5 else np.zeros((H, 5), dtype=np.int32)
        out.append(ransac_edge_both(p1, p2, K_TEST, samples, THRESHOLD, MARGIN))
    return out


def exact_cases():
    """200 edges of 8 noise-free pairs, general then sideways -> (pts1, pts2, edge_ptr, E_true (200, 3, 3))."""
    rng = np.random.default_rng(2702)
    edges, Et = [], []
    for kind in ("general", "sideways"):
        for _ in range(100):
            p1, p2, E, _, _, _ = scene(rng, 8, K_TEST, kind)
            edges.append((p1, p2))
            Et.append(E)
    return batch(edges) + (np.array(Et),)


def noisy_scene():
    """The end-to-end scene: 300 pairs, 0.3 px, 25 % outliers -> (pts1, pts2, R, t)."""
    p1, p2, _, R, t, _ = scene(np.random.default_rng(2703), 300, K_TEST, "general", noise=0.3, outliers=0.25)
    return p1, p2, R, t


def pose_errors(R, t, R_true, t_true):
    """-> (rotation error, angle between the translation directions), radians."""
    c = float(np.dot(t, t_true) / (np.linalg.norm(t) * np.linalg.norm(t_true)))
    return tv.rotation_angle(R, R_true), float(np.arccos(np.clip(c, -1.0, 1.0)))


def pair_edges():
    """Four edges for select_initial_pair: baselines 0.02, 0.5, 1.0, 2.0 over the same kind of scene (150 pairs, 0.3 px, 20 % outliers)."""
    rng = np.random.default_rng(2704)
    return [make_pairs(rng, 150, K_TEST, noise=0.3, outliers=0.2, baseline=b)[:2] for b in (0.02, 0.5, 1.0, 2.0)]


def initial_pair_choice(edges, H, seed, min_angle=3, max_angle=60):
    """The choice of select_initial_pair(two_view="essential") driven by the restatement -> the edge or None."""
    best, best_median = None, np.inf
    for e, (p1, p2) in enumerate(edges):
        est = ransac_edge(p1, p2, K_TEST, draw_samples5(seed, e, H, len(p1)), THRESHOLD)
        if est["status"] != OK:
            continue
        m = est["mask"]
        pose = tv.recover_pose_edge(est["E"], p1[m], p2[m], K_TEST)
        if pose["status"] != tv.OK or not pose["mask"].any():
            continue
        median = float(np.median(pose["angle_deg"][pose["mask"]]))
        if min_angle < median < max_angle and median < best_median:
            best, best_median = e, median
    return best
