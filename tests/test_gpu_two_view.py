"""GPU tests of sfmba_fundamental_ransac (k_fund_ransac, k_fund_finish) and sfmba_recover_pose (k_recover_pose): against
the reference's recorded output, against the numpy restatement where no reference output can exist, the sizes at which the
kernels take another path, every status, masks, determinism, isolation from the solver, and the Python helpers.

Bounds.  Counts, masks and the best hypothesis are compared EXACTLY: the fixtures' generator asserts that no recorded
distance lies within 1e-6 x threshold of the threshold, and with device-drawn samples a hypothesis is left out of the
comparison when the restatement finds one of its distances that close (at most 1 % of them may be).  F, R and t: the
restatement's own distance to the reference times 100 (tests/golden/two_view_bounds.json).  A point X of the two-view DLT is
the dehomogenised smallest eigenvector w of the 4x4 matrix M = A^T A: forming M rounds each entry by a few eps |M|, which
moves w by at most |dM| / (l2 - l1) (the gap of the two smallest eigenvalues), and X = w[:3] / w[3] moves by |dw| |(X, 1)|^2;
both sides do this once, so the bound is 64 eps l4 / (l2 - l1) |(X, 1)|^2 per point.  angle_deg: 1e-9 degrees against
numpy on the device's own X, R, t.  F_refit on scenes that are no fixtures (there the recorded bound holds, which was measured
on the fixtures' inliers only): the null vector f of the n x 9 matrix A of the inliers moves by |d(A^T A)| / (l2 - l1), with
|d(A^T A)| a few eps l9 from forming the 45 sums in another order, and the unit-norm F = T2^T f T1 / |T2^T f T1| by at most
2 |T1| |T2| / |T2^T f T1| times that: 64 eps l9 / (l2 - l1) 2 |T1| |T2| / |T2^T f T1|.

A best hypothesis with fewer than 8 inliers (the fixture's n = 8 at 0.05 px: eight noisy pairs no longer fit their own F
after the rank-2 step) is DEGENERATE by the header's definition: F is withheld, the counts, the best h and the mask are
still compared exactly."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

import two_view_ref as tv
from kernel_source import kernel_constant

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
BOUNDS = json.load(open(os.path.join(GOLDEN, "two_view_bounds.json")))
F_BOUND = BOUNDS["F_hyp"]["bound"]
K = np.array([[2905.88, 0.0, 1416.0], [0.0, 2905.88, 1064.0], [0.0, 0.0, 1.0]])
EST_FIELDS = ("F", "F_refit", "inlier_mask", "inliers", "best", "success", "status", "hyp_inliers")
POSE_FIELDS = ("R", "t", "front_mask", "X", "angle_deg", "front", "front_all", "sum_err", "status")


@pytest.fixture(scope="module")
def be():
    import sfmba
    b = sfmba.Backend(0)
    yield b
    b.close()


@pytest.fixture(scope="module")
def cases():
    return tv.load_cases(GOLDEN)


def batch(edges):
    """[(pts1, pts2), ...] -> pts1, pts2, edge_ptr"""
    ptr = np.concatenate([[0], np.cumsum([len(a) for a, _ in edges])]).astype(np.int64)
    return (np.concatenate([a for a, _ in edges]).reshape(-1, 2), np.concatenate([b for _, b in edges]).reshape(-1, 2), ptr)


def same_bits(a, b, fields):
    for name in fields:
        x, y = getattr(a, name), getattr(b, name)
        assert (x is None and y is None) or x.tobytes() == y.tobytes(), name


def refit_tolerance(p1, p2):
    """The bound of F_refit against the restatement on a scene that is no fixture (see the module's text)."""
    n1, T1 = tv.normalise(p1)
    n2, T2 = tv.normalise(p2)
    A = tv.matrix_A(n1, n2)
    lam = np.linalg.eigvalsh(A.T @ A)
    return (64 * EPS * lam[-1] / (lam[1] - lam[0]) * 2.0 * np.linalg.norm(T1, 2) * np.linalg.norm(T2, 2) /
            np.linalg.norm(tv.estimate_F(p1, p2)))


def check_edge_against_restatement(est, e, p1, p2, samples, thr, refit=False, confidence=0.99):
    """Edge e of a device result against the restatement on the same samples -> the number of hypotheses left out."""
    ref = tv.ransac_edge(p1, p2, samples, threshold=thr, confidence=confidence, refit=refit, margin=1e-6 * thr)
    sl = slice(int(est.edge_ptr[e]), int(est.edge_ptr[e + 1]))
    keep = ~ref["near"]
    assert np.array_equal(est.hyp_inliers[e][keep], ref["hyp"][keep]), e
    if not ref["near"].any():
        assert est.status[e] == ref["status"] and est.best[e] == ref["best"] and est.inliers[e] == ref["inliers"], e
        assert np.array_equal(est.inlier_mask[sl], ref["mask"]) and bool(est.success[e]) == ref["success"], e
        if ref["status"] == tv.OK:
            assert np.abs(est.F[e] - ref["F"]).max() <= F_BOUND, e
            tol = refit_tolerance(p1[ref["mask"]], p2[ref["mask"]]) if refit else F_BOUND
            assert np.abs(est.F_refit[e] - ref["F_refit"]).max() <= tol, e
            assert abs(np.linalg.norm(est.F[e]) - 1.0) <= 8 * EPS and est.F[e].ravel()[np.argmax(np.abs(est.F[e]))] > 0
        else:
            assert not est.F[e].any() and not est.F_refit[e].any()
    return int(ref["near"].sum())


# ---- against the reference ---------------------------------------------------------------------------------------------
def test_recorded_samples_against_the_reference(be, cases):
    ransac = cases[0]
    for thr in (0.1, 1.0):
        group = [c for c in ransac if c["threshold"] == thr]
        p1, p2, ptr = batch([(c["pts1"], c["pts2"]) for c in group])
        est = be.fundamental_ransac(p1, p2, edge_ptr=ptr, samples=np.stack([c["samples"] for c in group]), threshold=thr,
                                    refit=1, want_hyp=True)
        for e, c in enumerate(group):
            sl = slice(int(ptr[e]), int(ptr[e + 1]))
            assert np.array_equal(est.hyp_inliers[e], c["hyp_inliers"]), (c["n"], c["noise"])
            assert np.array_equal(est.inlier_mask[sl], c["mask"]) and est.inliers[e] == c["inliers"] and est.best[e] == c["best"]
            assert bool(est.success[e]) == c["success"]
            if c["inliers"] >= 8:
                assert est.status[e] == est.OK
                dF, dR = np.abs(est.F[e] - c["F"]).max(), np.abs(est.F_refit[e] - c["F_refit"]).max()
                print(f"n={c['n']} noise={c['noise']}: |F - ref| {dF:.2e} (bound {F_BOUND:.2e}), refit {dR:.2e} "
                      f"(bound {BOUNDS['F_refit']['bound']:.2e})")
                assert dF <= F_BOUND and dR <= BOUNDS["F_refit"]["bound"], (c["n"], c["noise"], dF, dR)
            else:
                assert est.status[e] == est.DEGENERATE and not est.F[e].any() and not est.F_refit[e].any()
        assert est.n_ok == sum(c["inliers"] >= 8 for c in group)


def test_pose_against_the_reference(be, cases):
    _, pose, Kg = cases
    p1, p2, ptr = batch([(c["pts1"], c["pts2"]) for c in pose])
    out = be.recover_pose(np.stack([c["E"] for c in pose]), p1, p2, Kg, edge_ptr=ptr)
    assert out.n_ok == len(pose)
    for e, c in enumerate(pose):
        sl = slice(int(ptr[e]), int(ptr[e + 1]))
        ang, dt = tv.rotation_angle(c["R"], out.R[e]), np.linalg.norm(c["t"] - out.t[e])
        print(f"n={c['n']} noise={c['noise']}: R {ang:.2e} rad (bound {BOUNDS['R_angle']['bound']:.2e}), t {dt:.2e} "
              f"(bound {BOUNDS['t_dist']['bound']:.2e})")
        assert out.status[e] == out.OK and ang <= BOUNDS["R_angle"]["bound"] and dt <= BOUNDS["t_dist"]["bound"]
        assert np.array_equal(out.front_mask[sl], c["mask"]) and out.front[e] == c["mask"].sum()
        win = int(np.argmax(out.front_all[e]))
        assert out.front_all[e][win] == out.front[e] and np.all(np.delete(out.front_all[e], win) < out.front[e])
        # X against the restatement's DLT with the device's own pose, point by point
        R, t = out.R[e], out.t[e]
        X = tv.dlt_points(Kg, R, t, c["pts1"], c["pts2"])
        M1 = Kg @ np.hstack([np.eye(3), np.zeros((3, 1))])
        M2 = Kg @ np.hstack([R, t.reshape(3, 1)])
        for i in range(c["n"]):
            A = np.array([c["pts1"][i, 0] * M1[2] - M1[0], c["pts1"][i, 1] * M1[2] - M1[1], c["pts2"][i, 0] * M2[2] - M2[0],
                          c["pts2"][i, 1] * M2[2] - M2[1]])
            lam = np.linalg.eigvalsh(A.T @ A)
            tol = 64 * EPS * lam[3] / (lam[1] - lam[0]) * (1.0 + X[i] @ X[i])
            assert np.abs(out.X[sl][i] - X[i]).max() <= tol, (c["n"], c["noise"], i)
        want = np.where(out.front_mask[sl], tv.ray_angles_deg(R, t, out.X[sl]), np.nan)
        assert np.array_equal(np.isnan(out.angle_deg[sl]), np.isnan(want))
        assert np.nanmax(np.abs(out.angle_deg[sl] - want)) <= 1e-9
        # the summed error: 4 n differences of pixel-sized numbers, each rounded to ~1e3 eps, through projections of condition ~1e1
        total = tv.reproj_total(Kg, R, t, out.X[sl], c["pts1"], c["pts2"])
        assert abs(out.sum_err[e] - total) <= 4 * c["n"] * 1e3 * EPS * 64, (out.sum_err[e], total)


# ---- against the restatement, device-drawn samples ----------------------------------------------------------------------
def test_drawn_samples_against_the_restatement_and_e_dependence(be):
    rng = np.random.default_rng(5)
    H, seed, thr = 100, 0xfedcba9876543210, 1.0
    edges = [tv.make_pairs(rng, 300, K, noise=0.3, outliers=0.25)[:2] for _ in range(3)]
    p1, p2, ptr = batch(edges)
    est = be.fundamental_ransac(p1, p2, edge_ptr=ptr, threshold=thr, max_iters=H, seed=seed, refit=1, want_hyp=True)
    left_out = 0
    for e, (a, b) in enumerate(edges):
        smp = tv.draw_samples(seed, e, H, len(a))
        left_out += check_edge_against_restatement(est, e, a, b, smp, thr, refit=True)
        # the documented e-dependence: edge e of the batch is a one-edge batch given that edge's samples
        one = be.fundamental_ransac(a, b, samples=smp, threshold=thr, refit=1, want_hyp=True)
        assert one.hyp_inliers[0].tobytes() == est.hyp_inliers[e].tobytes() and one.F[0].tobytes() == est.F[e].tobytes()
        assert one.F_refit[0].tobytes() == est.F_refit[e].tobytes() and one.best[0] == est.best[e]
        assert one.inlier_mask.tobytes() == est.inlier_mask[int(ptr[e]):int(ptr[e + 1])].tobytes()
    assert left_out <= 0.01 * 3 * H
    # ... and drawn as edge 0 of its own batch it differs from edge 1 of this one
    other = be.fundamental_ransac(*edges[1], threshold=thr, max_iters=H, seed=seed, want_hyp=True)
    assert other.hyp_inliers[0].tobytes() != est.hyp_inliers[1].tobytes()


def scene(rng, n):
    """An edge for the size tests: exact pixels up to 9 pairs, else 0.3 px of noise and 25 % outliers."""
    return tv.make_pairs(rng, n, K, noise=0.0 if n <= 9 else 0.3, outliers=0.0 if n <= 9 else 0.25)[:2]


def test_pair_counts_at_the_edges_of_the_loops(be):
    """n = 7 (FEW_PAIRS), 8, 9, around the wave's 64, where the workgroup's LDS passes 64 KiB, and at the LDS staging limit
    and one above it, in one batch with an empty edge in the middle."""
    L = kernel_constant("kTwoViewLdsPairs")
    rng = np.random.default_rng(11)
    sizes = [7, 8, 9, 63, 0, 64, 65, 1900, L, L + 1]          # (1900: staged pairs + the kernel's static LDS pass 64 KiB)
    edges = [scene(rng, n) if n else (np.zeros((0, 2)), np.zeros((0, 2))) for n in sizes]
    p1, p2, ptr = batch(edges)
    H, seed, thr = 24, 77, 1.0
    est = be.fundamental_ransac(p1, p2, edge_ptr=ptr, threshold=thr, max_iters=H, seed=seed, refit=1, want_hyp=True)
    left_out = 0
    for e, n in enumerate(sizes):
        if n < 8:
            assert est.status[e] == est.FEW_PAIRS and np.all(est.hyp_inliers[e] == -1) and est.best[e] == -1
            assert not est.F[e].any() and not est.inlier_mask[int(ptr[e]):int(ptr[e + 1])].any() and est.inliers[e] == 0
            continue
        left_out += check_edge_against_restatement(est, e, *edges[e], tv.draw_samples(seed, e, H, n), thr, refit=True)
    assert left_out <= 0.01 * H * len(sizes)
    assert est.n_ok == int((est.status == est.OK).sum()) >= 7


def test_hypothesis_counts_and_the_choice_between_slots(be):
    minslice = kernel_constant("kTwoViewMinSlice")
    rng = np.random.default_rng(12)
    a, b, _, _, bad = tv.make_pairs(rng, 64, K, noise=0.0, outliers=0.25)
    for H in (1, 63, 64, 65):
        est = be.fundamental_ransac(a, b, threshold=1.0, max_iters=H, seed=3, want_hyp=True)
        assert check_edge_against_restatement(est, 0, a, b, tv.draw_samples(3, 0, H, 64), 1.0) == 0
    # more hypotheses than one workgroup's slice can hold for ANY grid: H > minslice x (H / minslice) never happens, so
    # take H = 65 > 8 slices of 8: the best hypothesis planted in the last slot, then a tie planted in two slots
    H = 8 * minslice + 1
    clean, dirty = np.flatnonzero(~bad), np.flatnonzero(bad)
    smp = np.empty((H, 8), dtype=np.int32)
    for h in range(H):                                           # every sample holds an outlier ...
        smp[h] = np.concatenate([rng.choice(clean, 7, replace=False), rng.choice(dirty, 1)])
    smp[H - 1] = clean[:8]                                       # ... but the last
    est = be.fundamental_ransac(a, b, samples=smp, threshold=1.0, want_hyp=True)
    assert check_edge_against_restatement(est, 0, a, b, smp, 1.0) == 0
    assert est.best[0] == H - 1 and est.inliers[0] == len(clean) and np.array_equal(est.inlier_mask, ~bad)
    smp[10] = smp[H - 6] = clean[:8]                             # the same count in three slots: the lowest h wins
    est = be.fundamental_ransac(a, b, samples=smp, threshold=1.0, want_hyp=True)
    assert est.hyp_inliers[0][10] == est.hyp_inliers[0][H - 6] == est.hyp_inliers[0][H - 1] == len(clean)
    assert est.best[0] == 10 and check_edge_against_restatement(est, 0, a, b, smp, 1.0) == 0


def test_batches_of_one_two_and_257_edges(be):
    rng = np.random.default_rng(13)
    H, seed, thr = 16, 21, 1.0
    edges = [scene(rng, 20) for _ in range(257)]
    edges[128] = (np.zeros((0, 2)), np.zeros((0, 2)))
    for count in (1, 2, 257):
        p1, p2, ptr = batch(edges[:count])
        est = be.fundamental_ransac(p1, p2, edge_ptr=ptr, threshold=thr, max_iters=H, seed=seed, want_hyp=True)
        left_out = 0
        for e in range(count):
            if e == 128:
                assert est.status[e] == est.FEW_PAIRS
                continue
            left_out += check_edge_against_restatement(est, e, *edges[e], tv.draw_samples(seed, e, H, 20), thr)
        assert left_out <= 0.01 * H * count
        assert est.n_ok == int((est.status == est.OK).sum())
    # the pose call over the same 257 edges with the true E: every edge but the empty one OK
    rng = np.random.default_rng(14)
    made = [tv.make_pairs(rng, 20, K) for _ in range(257)]
    made[128] = (np.zeros((0, 2)), np.zeros((0, 2)), np.eye(3), np.array([1.0, 0.0, 0.0]), None)
    p1, p2, ptr = batch([(m[0], m[1]) for m in made])
    out = be.recover_pose(np.stack([tv.essential_from_pose(m[2], m[3]) for m in made]), p1, p2, K, edge_ptr=ptr)
    assert out.status[128] == out.FEW_PAIRS and out.n_ok == 256 and np.all(np.delete(out.front, 128) == 20)
    for e in (0, 127, 129, 256):
        assert tv.rotation_angle(made[e][2], out.R[e]) <= 1e-9 and np.linalg.norm(out.t[e] - made[e][3]) <= 1e-9


# ---- statuses -----------------------------------------------------------------------------------------------------------
def test_every_status(be):
    rng = np.random.default_rng(15)
    a, b, R, t, _ = tv.make_pairs(rng, 40, K)
    same = (np.tile(a[:1], (20, 1)), np.tile(b[:1], (20, 1)))
    p1, p2, ptr = batch([(a, b), (a[:7], b[:7]), same])
    est = be.fundamental_ransac(p1, p2, edge_ptr=ptr, threshold=0.1, max_iters=16, seed=1, want_hyp=True)
    assert est.status.tolist() == [est.OK, est.FEW_PAIRS, est.DEGENERATE] and est.n_ok == 1
    assert np.all(est.hyp_inliers[2] == 0) and not est.F[2].any() and not est.inlier_mask[47:].any()
    assert est.inliers[0] == 40 and est.success.tolist() == [True, False, False]
    # pose: OK, no pair, E = 0, E of rank 1, a NaN in E, and the mirrored scene
    E = tv.essential_from_pose(R, t)
    Y = np.stack([rng.uniform(-1.0, 1.0, 20), rng.uniform(-1.0, 1.0, 20), rng.uniform(4.0, 9.0, 20)], axis=1)
    Xm = np.concatenate([Y, -Y])                                 # half in front of both cameras, half behind both
    m1, m2 = Xm @ K.T, (Xm @ R.T + t) @ K.T
    m1, m2 = m1[:, :2] / m1[:, 2:3], m2[:, :2] / m2[:, 2:3]
    assert np.all((Y @ R.T + t)[:, 2] > 0) and np.all((-Y @ R.T + t)[:, 2] < 0)
    none = (np.zeros((0, 2)), np.zeros((0, 2)))
    p1, p2, ptr = batch([(a, b), none, (a, b), (a, b), (a, b), (m1, m2)])
    nanE = E.copy()
    nanE[1, 1] = np.nan
    Es = np.stack([E, E, np.zeros((3, 3)), np.outer([1.0, 2.0, 3.0], [0.5, -1.0, 2.0]), nanE, E])
    out = be.recover_pose(Es, p1, p2, K, edge_ptr=ptr)
    assert out.status.tolist() == [out.OK, out.FEW_PAIRS, out.DEGENERATE, out.DEGENERATE, out.DEGENERATE, out.TIE]
    assert out.n_ok == 1 and out.front[0] == 40
    for e in (2, 3, 4):
        sl = slice(int(ptr[e]), int(ptr[e + 1]))
        assert not out.R[e].any() and not out.t[e].any() and not out.front_mask[sl].any() and out.front[e] == 0
        assert np.isnan(out.X[sl]).all() and np.isnan(out.angle_deg[sl]).all() and np.isnan(out.sum_err[e])
    # the mirrored scene: (R, t) sees the first half in front, (R, -t) the second; the earlier candidate is returned
    top = np.sort(out.front_all[5])[::-1]
    assert top[0] == top[1] == 20 and out.front[5] == 20
    win = int(np.argmax(out.front_all[5]))
    assert out.front_all[5][win] == 20 and np.all(out.front_all[5][:win] < 20)
    ref = tv.recover_pose_edge(E, m1, m2, K)
    assert ref["status"] == tv.TIE and np.array_equal(ref["front_all"], out.front_all[5])
    assert np.array_equal(out.front_mask[int(ptr[5]):], ref["mask"])
    # min_depth moves the verdict of a pair
    deep = be.recover_pose(E, a, b, K, min_depth=6.5)
    assert 0 < deep.front[0] < 40 and np.array_equal(deep.front_mask, (out.X[:40, 2] > 6.5) & ((out.X[:40] @ R.T + t)[:, 2] > 6.5))


# ---- masks, samples ---------------------------------------------------------------------------------------------------------
def test_pair_use_equals_the_batch_without_those_pairs(be):
    rng = np.random.default_rng(16)
    made = [tv.make_pairs(rng, n, K, noise=0.3, outliers=0.25) for n in (90, 70)]
    p1, p2, ptr = batch([(m[0], m[1]) for m in made])
    use = rng.uniform(size=len(p1)) > 0.3
    use[ptr[1] - 1] = False
    kept_ptr = np.array([0, use[:ptr[1]].sum(), use.sum()], dtype=np.int64)
    smp = np.stack([tv.draw_samples(9, e, 24, int(kept_ptr[e + 1] - kept_ptr[e])) for e in range(2)])
    for kw in (dict(samples=smp), dict(max_iters=24, seed=9)):
        full = be.fundamental_ransac(p1, p2, edge_ptr=ptr, pair_use=use, threshold=1.0, refit=1, want_hyp=True, **kw)
        cut = be.fundamental_ransac(p1[use], p2[use], edge_ptr=kept_ptr, threshold=1.0, refit=1, want_hyp=True, **kw)
        same_bits(full, cut, ("F", "F_refit", "inliers", "best", "success", "status", "hyp_inliers"))
        assert np.array_equal(full.inlier_mask[use], cut.inlier_mask) and not full.inlier_mask[~use].any()
    Es = np.stack([tv.essential_from_pose(m[2], m[3]) for m in made])
    full = be.recover_pose(Es, p1, p2, K, edge_ptr=ptr, pair_use=use)
    cut = be.recover_pose(Es, p1[use], p2[use], K, edge_ptr=kept_ptr)
    same_bits(full, cut, ("R", "t", "front", "front_all", "sum_err", "status"))
    assert full.X[use].tobytes() == cut.X.tobytes() and full.angle_deg[use].tobytes() == cut.angle_deg.tobytes()
    assert np.array_equal(full.front_mask[use], cut.front_mask) and not full.front_mask[~use].any()
    assert np.isnan(full.X[~use]).all() and np.isnan(full.angle_deg[~use]).all()


def test_repeated_and_out_of_range_samples(be):
    rng = np.random.default_rng(17)
    a, b = tv.make_pairs(rng, 30, K)[:2]
    smp = tv.draw_samples(4, 0, 12, 30)
    smp[5, 7] = smp[5, 0]
    est = be.fundamental_ransac(a, b, samples=smp, threshold=0.1, want_hyp=True)
    assert est.hyp_inliers[0][5] == -1 and np.all(np.delete(est.hyp_inliers[0], 5) == 30) and est.best[0] == 0
    for bad in (30, -1):
        smp2 = smp.copy()
        smp2[3, 2] = bad
        with pytest.raises(ValueError):
            be.fundamental_ransac(a, b, samples=smp2, threshold=0.1)
    with pytest.raises(ValueError):
        be.fundamental_ransac(a, b, max_iters=0)
    with pytest.raises(ValueError):
        be.fundamental_ransac(a, b, threshold=np.nan)
    with pytest.raises(TypeError):
        be.fundamental_ransac(a, b, iterations=3)
    with pytest.raises(ValueError):
        be.fundamental_ransac(a, b, samples=smp, max_iters=11)


# ---- determinism ------------------------------------------------------------------------------------------------------------
def test_same_bits_twice_and_in_a_split_batch(be):
    rng = np.random.default_rng(18)
    made = [tv.make_pairs(rng, n, K, noise=0.3, outliers=0.25) for n in (80, 150, 64, 200)]
    edges = [(m[0], m[1]) for m in made]
    p1, p2, ptr = batch(edges)
    H = 40
    smp = np.stack([tv.draw_samples(2, e, H, len(edges[e][0])) for e in range(4)])
    kw = dict(threshold=1.0, refit=1, want_hyp=True, profile=1)
    one = be.fundamental_ransac(p1, p2, edge_ptr=ptr, samples=smp, **kw)
    two = be.fundamental_ransac(p1, p2, edge_ptr=ptr, samples=smp, **kw)
    same_bits(one, two, EST_FIELDS)
    assert one.kernel_us > 0.0
    drawn = [be.fundamental_ransac(p1, p2, edge_ptr=ptr, max_iters=H, seed=6, threshold=1.0, want_hyp=True) for _ in range(2)]
    same_bits(drawn[0], drawn[1], EST_FIELDS)
    for lo, hi in ((0, 1), (1, 4)):                              # the batch in two parts, the samples passed along
        q1, q2, qptr = batch(edges[lo:hi])
        part = be.fundamental_ransac(q1, q2, edge_ptr=qptr, samples=smp[lo:hi], **kw)
        for name in ("F", "F_refit", "inliers", "best", "success", "status", "hyp_inliers"):
            assert getattr(part, name).tobytes() == getattr(one, name)[lo:hi].tobytes(), name
        assert part.inlier_mask.tobytes() == one.inlier_mask[int(ptr[lo]):int(ptr[hi])].tobytes()
    Es = np.stack([tv.essential_from_pose(m[2], m[3]) for m in made])
    a = be.recover_pose(Es, p1, p2, K, edge_ptr=ptr, profile=1)
    b = be.recover_pose(Es, p1, p2, K, edge_ptr=ptr)
    same_bits(a, b, POSE_FIELDS)
    assert a.kernel_us > 0.0 and b.kernel_us == 0.0
    part = be.recover_pose(Es[1:], *batch(edges[1:])[:2], K, edge_ptr=batch(edges[1:])[2])
    assert part.R.tobytes() == a.R[1:].tobytes() and part.X.tobytes() == a.X[int(ptr[1]):].tobytes()


# ---- isolation ---------------------------------------------------------------------------------------------------------------
def test_two_view_calls_need_no_problem_and_do_not_disturb_a_solve():
    import sfmba
    rng = np.random.default_rng(19)
    a, b, R, t, _ = tv.make_pairs(rng, 120, K, noise=0.3, outliers=0.25)
    E = tv.essential_from_pose(R, t)
    pb = sfmba.make_problem(8, 120, 900, seed=21)

    def two_view(bk):
        est = bk.fundamental_ransac(a, b, max_iters=32, seed=1, refit=1)
        pose = bk.recover_pose(E, a, b, K, pair_use=est.inlier_mask)
        return est, pose

    def solve(bk, before=False, between=False):
        got = None
        if before:
            got = two_view(bk)                                   # no problem has been set on this handle yet
        bk.set_precision(64)
        bk.set_problem(*pb.args)
        opt = bk.default_options()
        opt.ftol = 1e-10
        xs, res, _, _ = bk.solve(pb.x0, opt, want_fun=False, want_grad=False)     # fun, grad stay on the device
        if between:
            kept = bk.fetch_fun_grad()
            got = two_view(bk)
            after = bk.fetch_fun_grad()
            assert kept[0].tobytes() == after[0].tobytes() and kept[1].tobytes() == after[1].tobytes()
        fun, grad = bk.fetch_fun_grad()
        return (xs, res.cost, int(res.nfev), fun, grad, bk.pcg_history()), got

    results = []
    for kw in (dict(), dict(between=True), dict(before=True)):
        bk = sfmba.Backend(0)
        try:
            results.append(solve(bk, **kw))
        finally:
            bk.close()
    want = results[0][0]
    for got, _ in results[1:]:
        assert got[0].tobytes() == want[0].tobytes() and got[1] == want[1] and got[2] == want[2]
        assert got[3].tobytes() == want[3].tobytes() and got[4].tobytes() == want[4].tobytes() and got[5] == want[5]
    # with and without a problem (and in fp32 storage) the two-view results are the same bits
    same_bits(results[1][1][0], results[2][1][0], EST_FIELDS[:-1])
    same_bits(results[1][1][1], results[2][1][1], POSE_FIELDS)
    assert results[2][1][0].status[0] == 0 and results[2][1][1].status[0] == 0
    bk = sfmba.Backend(0)
    try:
        bk.set_precision(32)
        bk.set_problem(*pb.args)
        est32, pose32 = two_view(bk)
    finally:
        bk.close()
    same_bits(est32, results[2][1][0], EST_FIELDS[:-1])
    same_bits(pose32, results[2][1][1], POSE_FIELDS)


# ---- the Python helpers --------------------------------------------------------------------------------------------------------
def test_cv2_style_helpers_and_the_initial_pair(be):
    import sfmba
    rng = np.random.default_rng(20)
    made = [tv.make_pairs(rng, 200, K, noise=0.3, outliers=0.2, baseline=bl, t_dir=(1.0, 0.2, 0.0)) for bl in (0.11, 1.15, 18.0)]
    medians = []
    for p1, p2, R, t, bad in made:                               # what the scene itself says: ~1, ~10 and ~70 degrees
        X = tv.dlt_points(K, R, t, p1[~bad], p2[~bad])
        medians.append(float(np.median(tv.ray_angles_deg(R, t, X))))
    assert 0.7 <= medians[0] <= 1.3 and 7.0 <= medians[1] <= 13.0 and 63.0 <= medians[2] <= 77.0, medians
    idx, R, t, X, mask = sfmba.select_initial_pair([(m[0], m[1]) for m in made], K, backend=be, max_iters=64, seed=1)
    assert idx == 1
    assert tv.rotation_angle(made[1][2], R) <= 1e-2 and np.linalg.norm(t - made[1][3] / np.linalg.norm(made[1][3])) <= 5e-2
    assert X.shape == (200, 3) and mask.shape == (200,) and np.isfinite(X[mask]).all() and np.isnan(X[~mask]).all()
    # ... which is the two batched calls, the second over the inliers of the first, and a host median
    p1, p2, ptr = batch([(m[0], m[1]) for m in made])
    est = be.fundamental_ransac(p1, p2, edge_ptr=ptr, max_iters=64, seed=1, refit=1)
    pose = be.recover_pose(np.einsum("ji,ejk,kl->eil", K, est.F_refit, K), p1, p2, K, edge_ptr=ptr, pair_use=est.inlier_mask)
    assert R.tobytes() == pose.R[1].tobytes() and t.tobytes() == pose.t[1].tobytes()
    assert np.array_equal(mask, pose.front_mask[200:400]) and mask.sum() == pose.front[1] == est.inliers[1] >= 8
    got = [float(np.median(pose.angle_deg[200 * e:200 * e + 200][pose.front_mask[200 * e:200 * e + 200]])) for e in range(3)]
    assert got[0] < 3.0 <= got[1] <= 60.0 < got[2], got
    # no edge inside the window
    assert sfmba.select_initial_pair([(made[0][0], made[0][1]), (made[2][0], made[2][1])], K, backend=be, max_iters=64,
                                     seed=1) == (None, None, None, None, None)
    # the two cv2-style calls
    p1, p2, R_true, t_true, bad = made[1]
    F, fmask = sfmba.find_fundamental_mat(p1, p2, ransacReprojThreshold=1.0, maxIters=64, seed=1, backend=be)
    est = be.fundamental_ransac(p1, p2, threshold=1.0, max_iters=64, seed=1, refit=1)
    assert F.shape == (3, 3) and fmask.shape == (200, 1) and fmask.dtype == np.uint8 and set(np.unique(fmask)) <= {0, 1}
    assert F.tobytes() == est.F_refit[0].tobytes() and np.array_equal(fmask.ravel() != 0, est.inlier_mask)
    assert fmask.sum() == est.inliers[0] >= 8
    Et = tv.essential_from_pose(R_true, t_true)
    n_front, R, t, pmask = sfmba.recover_pose(Et, p1[~bad], p2[~bad], K, backend=be)
    assert n_front == (~bad).sum() and pmask.shape == (n_front, 1) and np.all(pmask == 255) and t.shape == (3, 1)
    assert tv.rotation_angle(R_true, R) <= 1e-9 and np.linalg.norm(t.ravel() - t_true / np.linalg.norm(t_true)) <= 1e-9
