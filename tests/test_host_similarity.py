"""Host tests of the similarity feature (no GPU): the numpy restatement tests/similarity_ref.py against the oracle's
Umeyama fit, its tolerance, `apply_similarity`, `check_similarity_inputs` and the three-draw sample rule."""
import numpy as np
import pytest

import similarity_ref as sr

EPS = np.finfo(np.float64).eps


def oracle():
    from oracle import ba_oracle
    return ba_oracle


def umeyama(src, dst):
    """oracle.similarity_align on bare point sets -> (s, R, t)"""
    n = len(src)
    return oracle().similarity_align(np.asarray(src).ravel(), np.asarray(dst).ravel(), 0, n)[1]


def random_similarity(rng, angle=None):
    w = rng.normal(size=3)
    return (float(rng.uniform(0.5, 3.0)), sr.rodrigues(w * ((rng.uniform(0.2, 3.0) if angle is None else angle) / np.linalg.norm(w))),
            rng.normal(size=3) * 5.0)


# ---- Horn (eigh) against Umeyama (SVD) ------------------------------------------------------------------------------------
def test_horn_equals_the_oracles_umeyama_within_the_tolerance():
    """Two numpy routes to one estimate: Horn's quaternion by eigh (the restatement) and the oracle's SVD.  Both stay
    within estimate_tolerance of each other; the largest ratio met is printed (0.0877 on the machine this was written on)
    and goes into the docstring of tests/test_gpu_similarity.py."""
    rng = np.random.default_rng(7)
    worst = 0.0
    for n in (3, 4, 10, 300):
        for noise in (0.0, 0.01):
            for _ in range(5):
                src, dst, _, _ = sr.similar_sets(rng, n, noise=noise)
                got, want = sr.horn(src, dst), umeyama(src, dst)
                assert got is not None
                assert abs(np.linalg.det(got[1]) - 1.0) <= 16 * EPS and np.abs(got[1] @ got[1].T - np.eye(3)).max() <= 16 * EPS
                ratio = sr.tolerance_ratio(got, want, src, dst)
                worst = max(worst, ratio)
                # ... and in plain terms: s, R and t / |bm| agree to a few ulps
                assert abs(got[0] - want[0]) <= 64 * EPS * want[0] and np.abs(got[1] - want[1]).max() <= 64 * EPS
                assert np.abs(got[2] - want[2]).max() <= 256 * EPS * max(np.linalg.norm(dst.mean(axis=0)), 1.0)
    print(f"worst |Horn - Umeyama| / bound: {worst:.4f}")
    assert 0.0 < worst <= 1.0


def test_horn_has_no_solution_for_collinear_repeated_and_non_finite_triples():
    rng = np.random.default_rng(8)
    src, dst, _, _ = sr.similar_sets(rng, 3)
    line = src[0] + np.outer([0.0, 1.0, 2.5], src[1] - src[0])
    assert sr.horn(line, dst) is None                            # the rotation about the line is free
    assert sr.horn(np.tile(src[:1], (3, 1)), dst) is None        # saa = 0
    assert sr.horn(src, np.tile(dst[:1], (3, 1))) is None        # s = 0
    bad = dst.copy()
    bad[1, 2] = np.nan
    assert sr.horn(src, bad) is None
    assert sr.horn(src, dst) is not None
    # a mirrored triple still has a proper similarity: three points lie in a plane
    got = sr.horn(src, dst * np.array([-1.0, 1.0, 1.0]))
    assert got is not None and sr.distances_sq(got, src, dst * np.array([-1.0, 1.0, 1.0])).max() < 1e-20


def test_ransac_set_statuses():
    rng = np.random.default_rng(9)
    src, dst, _, bad = sr.similar_sets(rng, 40, noise=0.0, outliers=0.25)
    smp = sr.draw_samples3(1, 0, 50, 40)
    out = sr.ransac_set(src, dst, smp, 0.05, refit=True, margin=1e-6 * 0.05)
    assert out["status"] == sr.OK and out["inliers"] == int((~bad).sum()) and np.array_equal(out["mask"], ~bad)
    assert out["best"] == int(np.argmax(out["hyp"])) and not out["near"].any()
    assert sr.ransac_set(src[:2], dst[:2], smp, 0.05)["status"] == sr.FEW_PAIRS
    rep = np.tile(np.array([[1, 2, 1]], dtype=np.int32), (4, 1))
    deg = sr.ransac_set(src, dst, rep, 0.05)
    assert deg["status"] == sr.DEGENERATE and deg["best"] == -1 and np.all(deg["hyp"] == -1)
    same = sr.ransac_set(np.tile(src[:1], (9, 1)), np.tile(dst[:1], (9, 1)), sr.draw_samples3(1, 0, 4, 9), 0.05)
    assert same["status"] == sr.DEGENERATE and same["best"] == 0 and np.all(same["hyp"] == 0) and same["inliers"] == 0


# ---- apply_similarity ------------------------------------------------------------------------------------------------------
def ring(n_cameras=7, n_points=40, n_obs=200, seed=3):
    import sfmba
    return sfmba.make_ring_problem(n_cameras, n_points, n_obs, seed=seed)


def test_apply_similarity_equals_the_oracles_mapped_vector():
    import sfmba
    orc = oracle()
    rng = np.random.default_rng(10)
    for pb in (sfmba.make_problem(6, 60, 400, seed=21), ring()):
        C, P = pb.n_cameras, pb.n_points
        s, R, t = random_similarity(rng)
        pts = pb.x_true[6 * C:].reshape(P, 3)
        target = pb.x_true.copy()
        target[6 * C:] = (s * pts @ R.T + t).ravel()
        want, (s1, R1, t1) = orc.similarity_align(pb.x_true, target, C, P)
        got = sfmba.apply_similarity(pb.x_true, C, s1, R1, t1)
        mag = np.abs(want).max()
        # points and centres: the same expression; rotation vectors: both go matrix -> vector, to a few ulps of pi
        assert np.abs(got[6 * C:] - want[6 * C:]).max() <= 8 * EPS * mag
        gc, wc = got[:6 * C].reshape(C, 6), want[:6 * C].reshape(C, 6)
        assert np.abs(gc[:, 3:] - wc[:, 3:]).max() <= 8 * EPS * mag
        for c in range(C):
            assert np.abs(orc.rodrigues(gc[c:c + 1, :3])[0] - orc.rodrigues(wc[c:c + 1, :3])[0]).max() <= 64 * EPS


def test_residuals_do_not_change_under_a_similarity_and_the_inverse_returns_the_input():
    """The bound.  A mapped coordinate s R X + t carries 8 eps `mag` of rounding (three products, three sums, `mag` the
    largest mapped coordinate); the camera vector X' - T' therefore 16 eps mag, and the rotation R_c R^T, through
    the rotation vector and back, 32 eps times its length `reach`.  A pixel f x / z + c moves by f / depth (1 + |x / z|)
    times that, plus 8 eps of its own magnitude: in all 64 eps (f (mag + reach) / depth (1 + tan) + |pixel|), a factor of
    two over the sum of the terms."""
    import sfmba
    orc = oracle()
    rng = np.random.default_rng(11)
    worst = worst_back = 0.0
    for pb, angle in ((sfmba.make_problem(6, 60, 400, seed=21), None), (ring(), None), (ring(seed=4), 3.1)):
        C, P = pb.n_cameras, pb.n_points
        s, R, t = random_similarity(rng, angle)
        r0 = orc.compute_residuals(pb.x_true, *pb.args)
        y = sfmba.apply_similarity(pb.x_true, C, s, R, t)
        r1 = orc.compute_residuals(y, *pb.args)
        cams, pts = y[:6 * C].reshape(C, 6), y[6 * C:].reshape(P, 3)
        v = pts[pb.point_indices] - cams[pb.camera_indices, 3:]
        q = np.einsum("nij,nj->ni", orc.rodrigues(cams[:, :3])[pb.camera_indices], v)
        mag, reach, depth = np.abs(y).max(), np.linalg.norm(v, axis=1).max(), q[:, 2].min()
        tan = (np.abs(q[:, :2]) / q[:, 2:3]).max()
        pix = np.abs(pb.points_2d).max() + np.abs(r0).max()
        bound = 64 * EPS * (pb.K[0, 0] * (mag + reach) / depth * (1 + tan) + pix)
        assert depth > 0
        worst = max(worst, np.abs(r1 - r0).max() / bound)
        print(f"residual change {np.abs(r1 - r0).max():.3e} px (eps x pixel magnitude {EPS * pix:.3e}), bound {bound:.3e}")
        # the inverse similarity: X = (1/s) R^T X' - R^T t / s
        back = sfmba.apply_similarity(y, C, 1.0 / s, R.T, -(R.T @ t) / s)
        # (rotations compared as matrices: the ring's first camera is turned by exactly pi, where w and -w are one
        # rotation and either may come back)
        bound_back = 64 * EPS * (mag / s + np.abs(pb.x_true).max())
        bc, xc = back[:6 * C].reshape(C, 6), pb.x_true[:6 * C].reshape(C, 6)
        d = max(np.abs(back[6 * C:] - pb.x_true[6 * C:]).max(), np.abs(bc[:, 3:] - xc[:, 3:]).max())
        worst_back = max(worst_back, d / bound_back, np.abs(orc.rodrigues(bc[:, :3]) - orc.rodrigues(xc[:, :3])).max() / (64 * EPS))
        assert np.all(np.linalg.norm(bc[:, :3], axis=1) <= np.pi + 64 * EPS)
    print(f"worst residual change / bound {worst:.4f}; worst round trip / bound {worst_back:.4f}")
    assert 0.0 < worst <= 1.0 and 0.0 < worst_back <= 1.0


def test_apply_similarity_checks_its_arguments_and_keeps_nan_rows():
    import sfmba
    x = np.arange(6.0 * 2 + 9.0)
    x[6:12] = np.nan
    y = sfmba.apply_similarity(x, 2, 2.0, np.eye(3), [1.0, 0.0, 0.0])
    assert np.isnan(y[6:12]).all() and np.isfinite(y[:6]).all() and np.isfinite(y[12:]).all()
    assert np.array_equal(y[12:].reshape(3, 3), 2.0 * x[12:].reshape(3, 3) + [1.0, 0.0, 0.0])
    for bad in (dict(n_cameras=4), dict(R=np.eye(2)), dict(t=[1.0, 2.0])):
        kw = dict(n_cameras=2, s=1.0, R=np.eye(3), t=np.zeros(3))
        kw.update(bad)
        with pytest.raises(ValueError):
            sfmba.apply_similarity(x, kw["n_cameras"], kw["s"], kw["R"], kw["t"])


# ---- check_similarity_inputs -------------------------------------------------------------------------------------------------
def test_check_similarity_inputs():
    import sfmba
    src, dst = np.zeros((7, 3)), np.ones((7, 3))
    a, b, ptr, use, smp, opt = sfmba.check_similarity_inputs(src, dst, threshold=0.5)
    assert ptr.tolist() == [0, 7] and ptr.dtype == np.int64 and use is None and smp is None
    assert (opt.threshold, opt.confidence, opt.seed, opt.max_iters, opt.refit, opt.profile) == (0.5, 0.99, 0, 1000, 0, 0)
    a, b, ptr, use, smp, opt = sfmba.check_similarity_inputs(src.tolist(), dst, set_ptr=[0, 3, 3, 7], pair_use=[1, 0, 1, 1, 1, 1, 1],
                                                               samples=np.zeros((3, 5, 3), dtype=np.int64), seed=2 ** 64 - 1, refit=1)
    assert a.dtype == np.float64 and use.dtype == np.uint8 and use.tolist() == [1, 0, 1, 1, 1, 1, 1]
    assert smp.dtype == np.int32 and smp.shape == (3, 5, 3) and opt.max_iters == 5 and opt.seed == 2 ** 64 - 1 and opt.refit == 1
    assert sfmba.check_similarity_inputs(src, dst, samples=np.zeros((5, 3), dtype=np.int32))[4].shape == (1, 5, 3)
    for bad in (dict(src=np.zeros((7, 2))), dict(dst=np.ones((6, 3))), dict(set_ptr=[0, 5, 4, 7]), dict(set_ptr=[0, 6]),
                dict(set_ptr=[1, 7]), dict(pair_use=np.ones(6)), dict(samples=np.zeros((1, 5, 4), dtype=np.int32)),
                dict(samples=np.zeros((2, 5, 3), dtype=np.int32)), dict(samples=np.zeros((1, 5, 3), dtype=np.int32), max_iters=4),
                dict(threshold=np.nan), dict(confidence=np.nan), dict(max_iters=0), dict(seed=-1), dict(seed=2 ** 64)):
        kw = dict(src=src, dst=dst)
        kw.update(bad)
        with pytest.raises(ValueError):
            sfmba.check_similarity_inputs(**kw)
    with pytest.raises(TypeError):
        sfmba.check_similarity_inputs(src, dst, iterations=3)


def test_the_library_declares_and_binds_the_call():
    import os
    from conftest import ROOT
    from sfmba import _capi
    assert "sfmba_similarity_ransac" in _capi.SYMBOLS
    assert "int  sfmba_similarity_ransac(sfmba_handle* h, int64_t n_sets" in open(os.path.join(ROOT, "include", "sfmba.h")).read()


# ---- the draw rule ---------------------------------------------------------------------------------------------------------
PINNED = (                                                       # (seed, e, h, n) -> the triple, computed by the restatement
    ((0, 0, 0, 3), (1, 0, 2)),
    ((5, 1, 7, 4), (0, 1, 3)),
    ((0xfedcba9876543210, 2, 99, 300), (100, 193, 125)),
    ((1, 70000, 3, 5), (3, 0, 4)),
    ((9, 0, 12, 64), (30, 48, 28)),
)


def test_draw_rule_is_distinct_a_function_of_seed_e_h_and_pinned():
    for seed, e, n in ((0, 0, 3), (5, 1, 4), (0xfedcba9876543210, 2, 300), (1, 70000, 5)):
        smp = sr.draw_samples3(seed, e, 200, n)
        assert smp.shape == (200, 3) and smp.dtype == np.int32 and smp.min() >= 0 and smp.max() < n
        assert all(len(set(row)) == 3 for row in smp.tolist())
        # hypothesis h does not depend on how many are drawn, nor on the other sets
        assert np.array_equal(sr.draw_samples3(seed, e, 7, n), smp[:7]) and sr.draw_sample3(seed, e, 150, n) == smp[150].tolist()
    assert n_distinct_over_h(0, 0, 64, 10) > 32
    for (seed, e, h, n), want in PINNED:
        assert sr.draw_sample3(seed, e, h, n) == list(want), (seed, e, h, n)
    assert len(PINNED) == 5


def n_distinct_over_h(seed, e, H, n):
    return len({tuple(row) for row in sr.draw_samples3(seed, e, H, n).tolist()})
