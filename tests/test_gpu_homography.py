"""GPU tests of sfmba_homography_ransac (k_homog_ransac, k_homog_finish), of find_homography and of the H/F gate of
select_initial_pair: against the numpy restatement (tests/homography_ref.py; there is no reference code for H), the sizes
at which the kernels take another path, every status, masks, determinism, isolation from the F call and from the solver.

Bounds.  Counts, masks and the best hypothesis are compared EXACTLY; a hypothesis is left out of the comparison when the
restatement finds one of its distances within 1e-6 x threshold of the threshold (at most 1 % of them may be), and an
edge with such a hypothesis, or with such a distance of its H_refit, is skipped for the per-edge fields.  H and H_refit:
the null vector h of the 2n x 9 matrix A moves by |d(A^T A)| / (l2 - l1) (the gap of the two smallest eigenvalues of
A^T A), with |d(A^T A)| a few eps l9 from forming the sums in another order and from the Jacobi rotations, and the
unit-norm H = T2^-1 Hn T1 / |T2^-1 Hn T1| by at most 2 |T1| |T2^-1| / |T2^-1 Hn T1| times that:
64 eps l9 / (l2 - l1) 2 |T1| |T2^-1| / |T2^-1 Hn T1| (homography_ref.estimate_tolerance), the form of refit_tolerance in
tests/test_gpu_two_view.py.  Two numpy routes (eigh of A^T A, SVD of A with permuted rows) differ by at most 0.0098 of it."""
import numpy as np
import pytest

import homography_ref as hr
import two_view_ref as tv
from kernel_source import kernel_constant

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
K = np.array([[2905.88, 0.0, 1416.0], [0.0, 2905.88, 1064.0], [0.0, 0.0, 1.0]])
EST_FIELDS = ("H", "H_refit", "inlier_mask", "refit_mask", "inliers", "refit_inliers", "best", "success", "status", "hyp_inliers")
F_FIELDS = ("F", "F_refit", "inlier_mask", "inliers", "best", "success", "status", "hyp_inliers")
NONE = (np.zeros((0, 2)), np.zeros((0, 2)))
WORST = dict(ratio=0.0)                                          # the largest |H - restatement| / bound met by any test


@pytest.fixture(scope="module")
def be():
    import sfmba
    b = sfmba.Backend(0)
    yield b
    b.close()


def batch(edges):
    """[(pts1, pts2), ...] -> pts1, pts2, edge_ptr"""
    ptr = np.concatenate([[0], np.cumsum([len(a) for a, _ in edges])]).astype(np.int64)
    return (np.concatenate([a for a, _ in edges]).reshape(-1, 2), np.concatenate([b for _, b in edges]).reshape(-1, 2), ptr)


def same_bits(a, b, fields):
    for name in fields:
        x, y = getattr(a, name), getattr(b, name)
        assert (x is None and y is None) or x.tobytes() == y.tobytes(), name


def unit_and_sign(H):
    return abs(np.linalg.norm(H) - 1.0) <= 8 * EPS and H.ravel()[np.argmax(np.abs(H))] > 0


def check_edge(est, e, p1, p2, samples, thr, refit=True, confidence=0.99):
    """Edge e of a device result against the restatement on the same samples -> the number of hypotheses left out (an
    H_refit with a distance near the threshold counts as one)."""
    ref = hr.ransac_edge(p1, p2, samples, threshold=thr, confidence=confidence, refit=refit, margin=1e-6 * thr)
    sl = slice(int(est.edge_ptr[e]), int(est.edge_ptr[e + 1]))
    keep = ~ref["near"]
    assert np.array_equal(est.hyp_inliers[e][keep], ref["hyp"][keep]), e
    if ref["near"].any():
        return int(ref["near"].sum())
    assert est.status[e] == ref["status"] and est.best[e] == ref["best"] and est.inliers[e] == ref["inliers"], e
    assert np.array_equal(est.inlier_mask[sl], ref["mask"]) and bool(est.success[e]) == ref["success"], e
    if ref["status"] != hr.OK:
        assert not est.H[e].any() and not est.H_refit[e].any(), e
        assert np.array_equal(est.refit_mask[sl], ref["mask"]) and est.refit_inliers[e] == ref["inliers"], e
        return 0
    idx = np.asarray(samples)[ref["best"]]
    tol, d = hr.estimate_tolerance(p1[idx], p2[idx]), np.abs(est.H[e] - ref["H"]).max()
    WORST["ratio"] = max(WORST["ratio"], d / tol)
    assert d <= tol and unit_and_sign(est.H[e]), (e, d, tol)
    if not refit:
        assert est.H_refit[e].tobytes() == est.H[e].tobytes() and est.refit_mask[sl].tobytes() == est.inlier_mask[sl].tobytes()
        assert est.refit_inliers[e] == est.inliers[e]
        return 0
    m = ref["mask"]
    tol, d = hr.estimate_tolerance(p1[m], p2[m]), np.abs(est.H_refit[e] - ref["H_refit"]).max()
    WORST["ratio"] = max(WORST["ratio"], d / tol)
    assert d <= tol and unit_and_sign(est.H_refit[e]), (e, d, tol)
    if ref["near_refit"]:
        return 1
    assert np.array_equal(est.refit_mask[sl], ref["refit_mask"]) and est.refit_inliers[e] == ref["refit_inliers"], e
    return 0


# ---- 1: drawn samples against the restatement ---------------------------------------------------------------------------
def test_drawn_samples_against_the_restatement_and_e_dependence(be):
    rng = np.random.default_rng(41)
    H, seed, thr = 100, 0xfedcba9876543210, 1.0
    edges = [hr.planar_pairs(rng, 300, K, noise=0.3, outliers=0.25)[:2] for _ in range(3)]
    p1, p2, ptr = batch(edges)
    est = be.homography_ransac(p1, p2, edge_ptr=ptr, threshold=thr, max_iters=H, seed=seed, refit=1, want_hyp=True)
    left_out = 0
    for e, (a, b) in enumerate(edges):
        smp = hr.draw_samples4(seed, e, H, len(a))
        left_out += check_edge(est, e, a, b, smp, thr)
        # the documented e-dependence: edge e of the batch is a one-edge batch given that edge's samples
        one = be.homography_ransac(a, b, samples=smp[None], threshold=thr, refit=1, want_hyp=True)
        sl = slice(int(ptr[e]), int(ptr[e + 1]))
        assert one.hyp_inliers[0].tobytes() == est.hyp_inliers[e].tobytes() and one.H[0].tobytes() == est.H[e].tobytes()
        assert one.H_refit[0].tobytes() == est.H_refit[e].tobytes() and one.best[0] == est.best[e]
        assert one.inlier_mask.tobytes() == est.inlier_mask[sl].tobytes() and one.refit_mask.tobytes() == est.refit_mask[sl].tobytes()
        assert one.refit_inliers[0] == est.refit_inliers[e] and one.inliers[0] == est.inliers[e]
    print(f"left out: {left_out} of {3 * H} hypotheses")
    assert left_out <= 0.01 * 3 * H
    assert est.n_ok == 3 and np.all(est.refit_inliers >= 150)    # (most of the 225 clean pairs of 300: 0.3 px against 1 px)
    # ... and drawn as edge 0 of its own batch it differs from edge 1 of this one
    other = be.homography_ransac(*edges[1], threshold=thr, max_iters=H, seed=seed, want_hyp=True)
    assert other.hyp_inliers[0].tobytes() != est.hyp_inliers[1].tobytes()


# ---- 2: H and H_refit within the bound of the estimate's own conditioning ------------------------------------------------
def test_estimates_within_the_bound_of_their_conditioning(be):
    rng = np.random.default_rng(42)
    edges = []
    for n in (4, 5, 9, 64, 300):
        noise = 0.0 if n <= 5 else 0.3
        edges.append(hr.planar_pairs(rng, n, K, noise=noise)[:2])
        edges.append(hr.planar_pairs(rng, n, K, noise=noise, baseline=0.0)[:2])
        edges.append(tv.make_pairs(rng, n, K, noise=noise)[:2])
    p1, p2, ptr = batch(edges)
    H, seed, thr = 16, 5, 1.0
    before = WORST["ratio"]
    WORST["ratio"] = 0.0
    est = be.homography_ransac(p1, p2, edge_ptr=ptr, threshold=thr, max_iters=H, seed=seed, refit=1, want_hyp=True)
    left_out = sum(check_edge(est, e, a, b, hr.draw_samples4(seed, e, H, len(a)), thr) for e, (a, b) in enumerate(edges))
    print(f"worst |H - restatement| / bound over {2 * len(edges)} estimates: {WORST['ratio']:.4f}; left out {left_out}")
    assert est.n_ok == len(edges) and left_out <= 0.01 * H * len(edges) and 0.0 < WORST["ratio"] <= 1.0
    WORST["ratio"] = max(WORST["ratio"], before)


# ---- 3: sizes at which a path changes ---------------------------------------------------------------------------------------
def test_pair_counts_at_the_edges_of_the_loops(be):
    """n = 3 (FEW_PAIRS), 4, 5, around the wave's 64, where the workgroup's LDS passes 64 KiB, and at the LDS staging limit
    and one above it, in one batch with an empty edge in the middle."""
    L = kernel_constant("kTwoViewLdsPairs")
    rng = np.random.default_rng(43)
    sizes = [3, 4, 5, 63, 0, 64, 65, 1900, L, L + 1]          # (1900: staged pairs + the kernel's static LDS pass 64 KiB)
    edges = [hr.planar_pairs(rng, n, K, noise=0.0 if n <= 5 else 0.3, outliers=0.0 if n <= 5 else 0.25)[:2] if n else NONE
             for n in sizes]
    p1, p2, ptr = batch(edges)
    H, seed, thr = 24, 77, 1.0
    est = be.homography_ransac(p1, p2, edge_ptr=ptr, threshold=thr, max_iters=H, seed=seed, refit=1, want_hyp=True)
    left_out = 0
    for e, n in enumerate(sizes):
        sl = slice(int(ptr[e]), int(ptr[e + 1]))
        if n < 4:
            assert est.status[e] == est.FEW_PAIRS and np.all(est.hyp_inliers[e] == -1) and est.best[e] == -1
            assert not est.H[e].any() and not est.H_refit[e].any() and est.inliers[e] == 0 and est.refit_inliers[e] == 0
            assert not est.inlier_mask[sl].any() and not est.refit_mask[sl].any() and not est.success[e]
            continue
        left_out += check_edge(est, e, *edges[e], hr.draw_samples4(seed, e, H, n), thr)
    print(f"left out: {left_out} of {H * len(sizes)} hypotheses")
    assert left_out <= 0.01 * H * len(sizes)
    assert est.n_ok == int((est.status == est.OK).sum()) == 8
    assert est.inliers[1] == 4 and est.inliers[2] == 5           # exact pixels: every pair fits


# ---- 4: hypothesis counts and the choice between waves and slots ----------------------------------------------------------
def test_hypothesis_counts_and_the_choice_between_slots(be):
    minslice = kernel_constant("kTwoViewMinSlice")
    rng = np.random.default_rng(44)
    a, b, _, _, _, bad = hr.planar_pairs(rng, 64, K, noise=0.0, outliers=0.25)
    big = 8 * minslice + 1                                       # nine slices of a one-edge batch on any grid
    for H in (1, 3, 4, 5, minslice - 1, minslice + 1, big):
        est = be.homography_ransac(a, b, threshold=1.0, max_iters=H, seed=3, want_hyp=True)
        assert check_edge(est, 0, a, b, hr.draw_samples4(3, 0, H, 64), 1.0, refit=False) == 0
    H = big
    clean, dirty = np.flatnonzero(~bad), np.flatnonzero(bad)
    smp = np.empty((H, 4), dtype=np.int32)
    for h in range(H):                                           # every sample holds an outlier ...
        smp[h] = np.concatenate([rng.choice(clean, 3, replace=False), rng.choice(dirty, 1)])
    smp[H - 1] = clean[:4]                                       # ... but the last
    est = be.homography_ransac(a, b, samples=smp[None], threshold=1.0, want_hyp=True)
    assert check_edge(est, 0, a, b, smp, 1.0, refit=False) == 0
    assert est.best[0] == H - 1 and est.inliers[0] == len(clean) and np.array_equal(est.inlier_mask, ~bad)
    # the same sample set, so the same count, at several h: two waves of one slice (h = 13 in an earlier wave than h = 10),
    # other slices, the last slot -- the lowest h wins
    for h in (13, 10, 5 * minslice + 2, H - 6):
        smp[h] = clean[:4]
    est = be.homography_ransac(a, b, samples=smp[None], threshold=1.0, want_hyp=True)
    assert np.all(est.hyp_inliers[0][[10, 13, 5 * minslice + 2, H - 6, H - 1]] == len(clean))
    assert est.best[0] == 10 and check_edge(est, 0, a, b, smp, 1.0, refit=False) == 0


# ---- 5: caller samples ------------------------------------------------------------------------------------------------------
def test_repeated_and_out_of_range_samples_and_refit_off(be):
    rng = np.random.default_rng(45)
    a, b = hr.planar_pairs(rng, 30, K)[:2]
    smp = hr.draw_samples4(4, 0, 12, 30)
    smp[5, 3] = smp[5, 0]
    est = be.homography_ransac(a, b, samples=smp[None], threshold=0.1, want_hyp=True)
    assert est.hyp_inliers[0][5] == -1 and np.all(np.delete(est.hyp_inliers[0], 5) == 30) and est.best[0] == 0
    assert est.status[0] == est.OK
    # refit = 0 (the default): copies
    assert est.H_refit.tobytes() == est.H.tobytes() and est.refit_mask.tobytes() == est.inlier_mask.tobytes()
    assert est.refit_inliers.tobytes() == est.inliers.tobytes()
    # every sample repeated: DEGENERATE with no best hypothesis
    rep = np.tile(np.array([[1, 2, 3, 1]], dtype=np.int32), (12, 1))
    deg = be.homography_ransac(a, b, samples=rep[None], threshold=0.1, refit=1, want_hyp=True)
    assert deg.status[0] == deg.DEGENERATE and deg.best[0] == -1 and np.all(deg.hyp_inliers[0] == -1) and deg.n_ok == 0
    assert not deg.H.any() and not deg.H_refit.any() and not deg.inlier_mask.any() and not deg.refit_mask.any()
    assert deg.inliers[0] == 0 and deg.refit_inliers[0] == 0 and not deg.success[0]
    # four times the same pixel pair: hypotheses are valid, their H is not finite
    same = (np.tile(a[:1], (20, 1)), np.tile(b[:1], (20, 1)))
    flat = be.homography_ransac(*same, max_iters=8, seed=1, threshold=0.1, refit=1, want_hyp=True)
    assert flat.status[0] == flat.DEGENERATE and np.all(flat.hyp_inliers[0] == 0) and not flat.H.any() and flat.best[0] == 0
    # a position out of range: the call returns -1, which the binding raises as ValueError as for every call
    for bad in (30, -1):
        smp2 = smp.copy()
        smp2[3, 2] = bad
        with pytest.raises(ValueError, match="position"):
            be.homography_ransac(a, b, samples=smp2[None], threshold=0.1)
    with pytest.raises(ValueError):
        be.homography_ransac(a, b, max_iters=0)
    with pytest.raises(ValueError):
        be.homography_ransac(a, b, threshold=np.nan)
    with pytest.raises(TypeError):
        be.homography_ransac(a, b, iterations=3)
    with pytest.raises(ValueError):
        be.homography_ransac(a, b, samples=smp[None], max_iters=11)
    with pytest.raises(ValueError):
        be.homography_ransac(a, b, samples=tv.draw_samples(4, 0, 12, 30)[None])      # (1, H, 8): the F call's
    # the handle is still good
    assert be.homography_ransac(a, b, samples=smp[None], threshold=0.1).inliers[0] == 30


# ---- 6: a mask --------------------------------------------------------------------------------------------------------------
def test_pair_use_equals_the_batch_without_those_pairs(be):
    rng = np.random.default_rng(46)
    made = [hr.planar_pairs(rng, n, K, noise=0.3, outliers=0.25) for n in (90, 70)]
    p1, p2, ptr = batch([(m[0], m[1]) for m in made])
    use = rng.uniform(size=len(p1)) > 0.3
    use[ptr[1] - 1] = False
    kept_ptr = np.array([0, use[:ptr[1]].sum(), use.sum()], dtype=np.int64)
    smp = np.stack([hr.draw_samples4(9, e, 24, int(kept_ptr[e + 1] - kept_ptr[e])) for e in range(2)])
    for kw in (dict(samples=smp), dict(max_iters=24, seed=9)):
        full = be.homography_ransac(p1, p2, edge_ptr=ptr, pair_use=use, threshold=1.0, refit=1, want_hyp=True, **kw)
        cut = be.homography_ransac(p1[use], p2[use], edge_ptr=kept_ptr, threshold=1.0, refit=1, want_hyp=True, **kw)
        same_bits(full, cut, ("H", "H_refit", "inliers", "refit_inliers", "best", "success", "status", "hyp_inliers"))
        assert np.array_equal(full.inlier_mask[use], cut.inlier_mask) and not full.inlier_mask[~use].any()
        assert np.array_equal(full.refit_mask[use], cut.refit_mask) and not full.refit_mask[~use].any()
        assert cut.n_ok == 2 and cut.refit_inliers.min() >= 20


# ---- 7: determinism and isolation -------------------------------------------------------------------------------------------
def test_same_bits_twice_and_beside_the_fundamental_call(be):
    rng = np.random.default_rng(47)
    edges = [hr.planar_pairs(rng, n, K, noise=0.3, outliers=0.25)[:2] for n in (80, 150, 64, 200)]
    p1, p2, ptr = batch(edges)
    kw = dict(edge_ptr=ptr, threshold=1.0, max_iters=40, seed=6, refit=1, want_hyp=True)
    f0 = be.fundamental_ransac(p1, p2, **kw)
    one = be.homography_ransac(p1, p2, profile=1, **kw)
    f1 = be.fundamental_ransac(p1, p2, **kw)
    two = be.homography_ransac(p1, p2, **kw)
    same_bits(one, two, EST_FIELDS)
    same_bits(f0, f1, F_FIELDS)
    assert one.kernel_us > 0.0 and two.kernel_us == 0.0 and one.n_ok == 4
    # the batch in two parts, the samples passed along
    smp = np.stack([hr.draw_samples4(6, e, 40, len(edges[e][0])) for e in range(4)])
    for lo, hi in ((0, 1), (1, 4)):
        q1, q2, qptr = batch(edges[lo:hi])
        part = be.homography_ransac(q1, q2, edge_ptr=qptr, samples=smp[lo:hi], threshold=1.0, refit=1, want_hyp=True)
        for name in ("H", "H_refit", "inliers", "refit_inliers", "best", "success", "status", "hyp_inliers"):
            assert getattr(part, name).tobytes() == getattr(one, name)[lo:hi].tobytes(), name
        assert part.inlier_mask.tobytes() == one.inlier_mask[int(ptr[lo]):int(ptr[hi])].tobytes()
        assert part.refit_mask.tobytes() == one.refit_mask[int(ptr[lo]):int(ptr[hi])].tobytes()


def test_homography_calls_need_no_problem_and_do_not_disturb_a_solve():
    import sfmba
    rng = np.random.default_rng(48)
    a, b = hr.planar_pairs(rng, 120, K, noise=0.3, outliers=0.25)[:2]
    pb = sfmba.make_problem(6, 60, 400, seed=21)

    def solve(bk, beside):
        got = []
        if beside:
            got.append(bk.homography_ransac(a, b, max_iters=32, seed=1, refit=1))      # no problem has been set yet
        bk.set_precision(64)
        bk.set_problem(*pb.args)
        opt = bk.default_options()
        opt.ftol = 1e-10
        xs, res, _, _ = bk.solve(pb.x0, opt, want_fun=False, want_grad=False)          # fun, grad stay on the device
        if beside:
            got.append(bk.homography_ransac(a, b, max_iters=32, seed=1, refit=1))
        fun, grad = bk.fetch_fun_grad()
        return (xs, res.cost, int(res.nfev), fun, grad, bk.pcg_history()), got

    results = []
    for beside in (False, True):
        bk = sfmba.Backend(0)
        try:
            results.append(solve(bk, beside))
        finally:
            bk.close()
    want, got = results[0][0], results[1][0]
    assert got[0].tobytes() == want[0].tobytes() and got[1] == want[1] and got[2] == want[2]
    assert got[3].tobytes() == want[3].tobytes() and got[4].tobytes() == want[4].tobytes() and got[5] == want[5]
    same_bits(results[1][1][0], results[1][1][1], EST_FIELDS[:-1])
    assert results[1][1][0].status[0] == 0


# ---- 8: model selection -----------------------------------------------------------------------------------------------------
def test_homography_gate_of_the_initial_pair_and_find_homography(be):
    """Scenes and seeds chosen on the CPU with the two restatements (300 pairs, 0.3 px, 25 % outliers, threshold 1 px, 100
    hypotheses, seed 1): generator seed 2 gives a planar edge whose F is OK with a median angle of 4.94 degrees, a general
    edge at 8.01 and a pure rotation at 0.01; the support ratios of the generator seeds 2..5 are 0.977-1.000 (planar),
    0.963-0.977 (pure rotation) and 0.020-0.040 (general)."""
    import sfmba
    kw = dict(threshold=1.0, max_iters=100, seed=1)
    ratios = dict(planar=[], general=[], rotation=[])
    for gen in (2, 3, 4, 5):
        rng = np.random.default_rng(gen)
        planar = hr.planar_pairs(rng, 300, K, noise=0.3, outliers=0.25, baseline=1.0)
        general = tv.make_pairs(rng, 300, K, noise=0.3, outliers=0.25)
        rotation = hr.planar_pairs(rng, 300, K, noise=0.3, outliers=0.25, baseline=0.0)
        edges = [(planar[0], planar[1]), (general[0], general[1]), (rotation[0], rotation[1])]
        p1, p2, ptr = batch(edges)
        F = be.fundamental_ransac(p1, p2, edge_ptr=ptr, refit=1, **kw)
        Hm = be.homography_ransac(p1, p2, edge_ptr=ptr, refit=1, **kw)
        assert np.all(F.inliers > 0)
        r = Hm.refit_inliers / F.inliers
        print(f"generator seed {gen}: H refit inliers / F inliers: planar {r[0]:.3f}, general {r[1]:.3f}, pure rotation {r[2]:.3f}")
        for name, v in zip(("planar", "general", "rotation"), r):
            ratios[name].append(float(v))
        if gen != 2:
            continue
        # today's rule starts from the planar edge; the gate passes it (and the rotation) over
        pose = be.recover_pose(np.einsum("ji,ejk,kl->eil", K, F.F_refit, K), p1, p2, K, edge_ptr=ptr, pair_use=F.inlier_mask)
        med = [float(np.median(pose.angle_deg[300 * e:300 * e + 300][pose.front_mask[300 * e:300 * e + 300]])) for e in range(3)]
        print(f"median ray angles: planar {med[0]:.2f}, general {med[1]:.2f}, pure rotation {med[2]:.2f} degrees")
        assert F.status.tolist() == [0, 0, 0] and pose.status[0] == pose.OK and pose.status[1] == pose.OK
        assert 3.0 < med[0] < 60.0 and med[0] <= med[1] - 1.0 and med[1] < 60.0
        today = sfmba.select_initial_pair(edges, K, backend=be, **kw)
        assert today[0] == 0
        same = sfmba.select_initial_pair(edges, K, backend=be, max_homography_ratio=None, **kw)
        assert same[0] == 0 and all(x.tobytes() == y.tobytes() for x, y in zip(today[1:], same[1:]))
        gated = sfmba.select_initial_pair(edges, K, backend=be, max_homography_ratio=0.5, **kw)
        assert gated[0] == 1
        assert tv.rotation_angle(general[2], gated[1]) <= 1e-2
        assert gated[1].tobytes() == pose.R[1].tobytes() and np.array_equal(gated[4], pose.front_mask[300:600])
        # a gate that nothing passes
        assert sfmba.select_initial_pair(edges, K, backend=be, max_homography_ratio=0.0, **kw) == (None,) * 5
        # find_homography on the planar edge
        H1, mask = sfmba.find_homography(planar[0], planar[1], ransacReprojThreshold=1.0, maxIters=100, seed=1, backend=be)
        one = be.homography_ransac(planar[0], planar[1], refit=1, **kw)
        assert H1.shape == (3, 3) and H1[2, 2] == 1.0 and mask.shape == (300, 1) and mask.dtype == np.uint8
        assert set(np.unique(mask)) <= {0, 1} and np.array_equal(mask.ravel() != 0, one.refit_mask)
        assert mask.sum() == one.refit_inliers[0] == Hm.refit_inliers[0]
        want = one.H_refit[0] / one.H_refit[0][2, 2]
        want[2, 2] = 1.0
        assert H1.tobytes() == want.tobytes() and one.H_refit[0].tobytes() == Hm.H_refit[0].tobytes()
        # ... which is the scene's homography: clean pairs transfer to within the noise
        d = np.sqrt(hr.distances_sq(H1, planar[0][~planar[5]], planar[1][~planar[5]]))
        assert np.median(d) < 1.0 and np.abs(hr.unit_H(H1) - hr.unit_H(planar[2])).max() < 1e-2
        none, mask0 = sfmba.find_homography(planar[0][:3], planar[1][:3], backend=be)
        assert none is None and mask0.shape == (3, 1) and not mask0.any()
    assert min(ratios["planar"]) > 0.8 and min(ratios["rotation"]) > 0.8 and max(ratios["general"]) < 0.2, ratios
