"""GPU tests of sfmba_resect_ransac (k_pnp_gather, k_pnp_ransac, k_pnp_finish, then k_resect over the inliers): the fixture
scenes against the numpy restatement and the reference's recorded pose, drawn samples, observation and hypothesis counts
at the loop edges, batches, every status, masks, storage precision, bitwise repeatability, isolation from the solver, the
drop-in wrapper and the timing entry.

Counts are compared exactly wherever the restatement does not flag a hypothesis `close` (pnp_ransac_ref.py); poses within
tests/golden/pnp_ransac_bounds.json: the best hypothesis within the minimal solver's bound (p3p_*) of the restatement's,
the final pose within final_* of the restatement's and of the reference's solve_pnp on the inlier set.  Two refinements
that both stop on xtol lie within 200 xtol (|p| + xtol) of each other (test_gpu_resect.py)."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

import pnp_ransac_ref as pr
import resect_ref as rr
from consumer_inputs import camera_slices_problem
from kernel_source import kernel_constant

pytestmark = pytest.mark.gpu

XTOL = 1e-10
BOUNDS = json.load(open(os.path.join(GOLDEN, "pnp_ransac_bounds.json")))
K = np.array([[2905.88, 0.0, 1416.0], [0.0, 2905.88, 1064.0], [0.0, 0.0, 1.0]])
FIELDS = ("cameras", "hyp", "inlier_mask", "status", "views", "inliers", "best", "best_sol", "success", "iters", "rms_err")


@pytest.fixture(scope="module")
def be():
    import sfmba
    b = sfmba.Backend(0)
    yield b
    b.close()


def set_problem(be, args, bits=64):
    be.set_precision(bits)
    be.set_fixed_cameras(())
    be.set_problem(*args)


def make_camera(rng, n, bad_share=0.3, noise=0.5):
    """A pose, n points 4..9 units in front of it, `noise` px of noise, a share of the pixels displaced by 20-200 px
    -> (X, uv, params, displaced)."""
    w = rng.normal(size=3)
    w *= rng.uniform(0.2, 1.0) / np.linalg.norm(w)
    T = rng.normal(0.0, 1.5, 3)
    cam = np.stack([rng.uniform(-1.8, 1.8, n), rng.uniform(-1.3, 1.3, n), rng.uniform(4.0, 9.0, n)], axis=1)
    uv = cam @ K.T
    uv = uv[:, :2] / uv[:, 2:3] + noise * rng.normal(size=(n, 2))
    bad = np.zeros(n, dtype=bool)
    bad[rng.choice(n, int(round(bad_share * n)), replace=False)] = True
    ang = rng.uniform(0.0, 2.0 * np.pi, n)
    uv[bad] += (rng.uniform(20.0, 200.0, n)[:, None] * np.stack([np.cos(ang), np.sin(ang)], axis=1))[bad]
    return cam @ rr.orc.rodrigues(w) + T, uv, np.concatenate([w, T]), bad


def build(cams, x_cams=None):
    """One problem of the cameras' own points -> (x, args, truth (C, 6), displaced (N))."""
    C = len(cams)
    n = [len(c[0]) for c in cams]
    ci = np.repeat(np.arange(C, dtype=np.int64), n)
    pi = np.arange(sum(n), dtype=np.int64)
    X = np.concatenate([c[0] for c in cams]).reshape(-1, 3)
    uv = np.concatenate([c[1] for c in cams]).reshape(-1, 2)
    truth = np.stack([c[2] for c in cams])
    x = np.concatenate([(np.full((C, 6), 0.25) if x_cams is None else x_cams).ravel(), X.ravel()])
    return x, (C, len(pi), ci, pi, uv, K), truth, np.concatenate([c[3] for c in cams])


def pose_gap(p, q):
    return rr.rotation_angle(rr.orc.rodrigues(q[:3]), rr.orc.rodrigues(p[:3])), float(np.linalg.norm(p[3:] - q[3:]))


def near(p, q, factor=200.0):
    return float(np.sqrt(((p - q) ** 2).sum())) <= factor * XTOL * (np.sqrt(q @ q) + XTOL)


def check_against(res, ref, ci, what="", poses=True):
    """Everything the restatement pins: every count where it is not close; a camera's best hypothesis, mask, verdict and
    poses unless a close hypothesis could be, or be level with, its best (a close count may be one off).  -> the number
    of cameras compared in full."""
    C = len(ref["status"])
    assert np.array_equal(res.views, ref["views"]), what
    if res.hyp_inliers is not None:
        sure = ~ref["hyp_close"]
        assert np.array_equal(res.hyp_inliers[sure], ref["hyp_inliers"][sure]), what
    n_sure = 0
    for c in range(C):
        b = ref["best"][c]
        if b >= 0 and ref["hyp_close"][c].any() and (ref["hyp_close"][c, b] or
                                                      ref["hyp_inliers"][c][ref["hyp_close"][c]].max() >= ref["inliers"][c] - 1):
            continue                                             # a close hypothesis may legitimately win or tie elsewhere
        n_sure += 1
        assert np.array_equal(res.inlier_mask[ci == c], ref["inlier_mask"][ci == c]), (what, c)
        for key in ("status", "best", "best_sol", "inliers", "success"):
            assert getattr(res, key)[c] == ref[key][c], (what, c, key, getattr(res, key)[c], ref[key][c])
        if poses and ref["best_sol"][c] >= 0:
            a, d = pose_gap(res.hyp[c], ref["hyp"][c])
            assert a <= BOUNDS["p3p_R_angle"]["bound"] and d <= BOUNDS["p3p_T_dist"]["bound"], (what, c, a, d)
        if poses and ref["status"][c] == pr.OK:
            a, d = pose_gap(res.cameras[c], ref["cameras"][c])
            assert a <= BOUNDS["final_R_angle"]["bound"] and d <= BOUNDS["final_T_dist"]["bound"], (what, c, a, d)
    return n_sure


# ---- the fixture scenes, the reason for the feature, the drop-in wrapper -----------------------------------------------------

def fixture_scenes():
    g = np.load(os.path.join(GOLDEN, "pnp_ransac_cases.npz"), allow_pickle=False)
    for k in range(len(g["n"])):
        sl = slice(int(g["ptr"][k]), int(g["ptr"][k + 1]))
        hs = slice(int(g["hptr"][k]), int(g["hptr"][k + 1]))
        yield dict(n=int(g["n"][k]), H=int(g["H"][k]), X=g["X"][sl], uv=g["uv"][sl], displaced=g["displaced"][sl],
                   samples=g["samples"][hs], K=g["K"], threshold=float(g["threshold"]), min_views=int(g["min_views"]),
                   rvec=g["rvec"][k], tvec=g["tvec"][k], rvec_true=g["rvec_true"][k], T_true=g["T_true"][k])


def test_fixture_scenes(be):
    import sfmba
    for sc in fixture_scenes():
        n, H = sc["n"], sc["H"]
        args = (1, n, np.zeros(n, dtype=np.int64), np.arange(n, dtype=np.int64), sc["uv"], sc["K"])
        x = np.concatenate([np.zeros(6), sc["X"].ravel()])
        opts = dict(threshold=sc["threshold"], min_views=sc["min_views"])
        set_problem(be, args)
        res = be.resect_ransac(x, samples=sc["samples"][None], want_hyp=True, **opts)
        ref = pr.resect_ransac(x, args, samples=sc["samples"][None], **opts)
        close = ref["hyp_close"][0]
        assert close.mean() <= 0.02 and not close[ref["best"][0]]
        assert np.array_equal(res.hyp_inliers[0][~close], ref["hyp_inliers"][0][~close])
        for key in ("status", "best", "best_sol", "inliers", "views", "success"):
            assert getattr(res, key)[0] == ref[key][0], (n, key)
        assert res.status[0] == res.OK and res.n_ok == 1
        assert np.array_equal(res.inlier_mask, ref["inlier_mask"]) and not np.any(res.inlier_mask & sc["displaced"])
        a, d = pose_gap(res.hyp[0], ref["hyp"][0])
        R_ref = rr.orc.rodrigues(sc["rvec"])
        p_ref = np.concatenate([sc["rvec"], -R_ref.T @ sc["tvec"]])
        a1, d1 = pose_gap(res.cameras[0], ref["cameras"][0])
        a2, d2 = pose_gap(res.cameras[0], p_ref)
        print(f"n={n} H={H}: {int(close.sum())} close; best hypothesis vs restatement R {a:.2e} T {d:.2e}; final vs restatement "
              f"R {a1:.2e} T {d1:.2e}, vs reference R {a2:.2e} T {d2:.2e}; {int(res.iters[0])} trial poses, rms {res.rms_err[0]:.3f} px")
        assert a <= BOUNDS["p3p_R_angle"]["bound"] and d <= BOUNDS["p3p_T_dist"]["bound"]
        assert max(a1, a2) <= BOUNDS["final_R_angle"]["bound"] and max(d1, d2) <= BOUNDS["final_T_dist"]["bound"]
        # the reason for the feature: plain resection over all observations has a high error or ends far from the truth
        truth = np.concatenate([sc["rvec_true"], sc["T_true"]])
        plain = sfmba.resect_cameras(x, args, backend=be, max_rms_px=2.0, min_depth=-np.inf)
        a3, d3 = pose_gap(plain.cameras[0], truth)
        assert plain.status[0] == plain.HIGH_ERROR or a3 > 100.0 * BOUNDS["final_R_angle"]["bound"] or d3 > 100.0 * BOUNDS["final_T_dist"]["bound"]
        rob = sfmba.resect_cameras_ransac(x, args, backend=be, samples=sc["samples"][None], **opts)
        assert rob.cameras.tobytes() == res.cameras.tobytes()
        # against the truth: the reference's own distance to it is the noise's, so the bound is relative to the reference
        a4, d4 = pose_gap(rob.cameras[0], p_ref)
        assert a4 <= BOUNDS["final_R_angle"]["bound"] and d4 <= BOUNDS["final_T_dist"]["bound"]
        # drop-in: OpenCV's convention, inliers = the mask's positions
        ok, rvec, tvec, inl = sfmba.solve_pnp_ransac(sc["X"], sc["uv"], sc["K"], None, iterationsCount=H, reprojectionError=sc["threshold"],
                                                     seed=3, backend=be, min_views=sc["min_views"])
        drawn = be.resect_ransac(x, max_iters=H, seed=3, **opts)
        assert ok and rvec.shape == (3, 1) and tvec.shape == (3, 1) and inl.dtype == np.int32 and inl.shape == (drawn.inliers[0], 1)
        assert np.array_equal(inl.ravel(), np.flatnonzero(drawn.inlier_mask)) and rvec.ravel().tobytes() == drawn.cameras[0, :3].tobytes()
        assert np.allclose(tvec.ravel(), -rr.orc.rodrigues(drawn.cameras[0, :3]) @ drawn.cameras[0, 3:], rtol=0, atol=1e-12)
    bad = sfmba.solve_pnp_ransac(np.zeros((8, 3)), np.zeros((8, 2)), K, backend=be)
    assert bad[0] is False and np.isnan(bad[1]).all() and np.isnan(bad[2]).all() and bad[3].shape == (0, 1)


# ---- drawn samples ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def three():
    rng = np.random.default_rng(17)
    return build([make_camera(rng, n) for n in (30, 70, 45)])


def test_drawn_samples(be, three):
    x, args, truth, bad = three
    set_problem(be, args)
    opts = dict(max_iters=48, threshold=2.0)
    a = be.resect_ransac(x, seed=5, want_hyp=True, **opts)
    ref = pr.resect_ransac(x, args, seed=5, **opts)
    assert check_against(a, ref, args[2], "seed 5") >= 2
    assert np.all(a.status == a.OK) and not np.any(a.inlier_mask & bad)
    b = be.resect_ransac(x, seed=6, want_hyp=True, **opts)
    assert not np.array_equal(a.hyp_inliers, b.hyp_inliers)
    assert check_against(b, pr.resect_ransac(x, args, seed=6, **opts), args[2], "seed 6") >= 2
    big = be.resect_ransac(x, seed=2 ** 64 - 1, want_hyp=True, **opts)
    assert check_against(big, pr.resect_ransac(x, args, seed=2 ** 64 - 1, **opts), args[2], "largest seed") >= 2
    # a camera's result does not depend on which others are selected
    sel = np.array([0, 1, 0], dtype=bool)
    one = be.resect_ransac(x, select=sel, seed=5, want_hyp=True, **opts)
    assert list(one.status) == [one.NOT_SELECTED, a.status[1], one.NOT_SELECTED]
    for name in FIELDS + ("hyp_inliers",):
        if name != "inlier_mask":                                # (per observation: below)
            assert getattr(one, name)[1].tobytes() == getattr(a, name)[1].tobytes(), name
    ci = args[2]
    assert np.array_equal(one.inlier_mask[ci == 1], a.inlier_mask[ci == 1]) and not one.inlier_mask[ci != 1].any()
    assert one.cameras[[0, 2]].tobytes() == x[:18].reshape(3, 6)[[0, 2]].tobytes() and np.all(one.hyp_inliers[[0, 2]] == -1)


# ---- observation counts at the loop edges ------------------------------------------------------------------------------------

def test_observation_counts_at_the_loop_edges(be):
    L = kernel_constant("kPnpLdsObs")
    assert kernel_constant("kPnpThreads") == 256 and L >= 512
    lengths = [3, 4, 5, 63, 64, 65, 255, 256, 257, L, L + 1]
    x, args = camera_slices_problem(lengths, seed=33)
    uv = args[4].copy()
    rng = np.random.default_rng(8)
    ptr = np.concatenate([[0], np.cumsum(lengths)])
    for c, n in enumerate(lengths):                              # a fifth of every camera's pixels displaced (from 5 observations on)
        k = ptr[c] + rng.choice(n, n // 5, replace=False)
        uv[k] += rng.uniform(30.0, 150.0, (len(k), 2))
    args = args[:4] + (uv, args[5])
    set_problem(be, args)
    opts = dict(max_iters=24, threshold=3.0, min_views=4, seed=11)
    res = be.resect_ransac(x, want_hyp=True, **opts)
    ref = pr.resect_ransac(x, args, **opts)
    assert list(res.views) == lengths and res.status[0] == res.FEW_VIEWS and np.all(res.hyp_inliers[0] == -1)
    assert res.cameras[0].tobytes() == x[:6].tobytes() and res.hyp[0].tobytes() == x[:6].tobytes() and np.isnan(res.rms_err[0])
    n_sure = check_against(res, ref, args[2], "loop edges")
    print(f"{n_sure} of {len(lengths)} cameras compared in full")
    assert n_sure >= len(lengths) // 2
    assert np.all(res.status[3:] == res.OK), res.status
    for c in range(1, len(lengths)):
        print(f"n={lengths[c]}: status {res.status[c]}, {res.inliers[c]} inliers (restatement {ref['inliers'][c]}), best {res.best[c]}.{res.best_sol[c]}")
        assert res.inlier_mask[ptr[c]:ptr[c + 1]].sum() == res.inliers[c]


# ---- hypothesis counts, planted winners, ties -------------------------------------------------------------------------------------

def test_hypothesis_counts_and_planted_winners(be):
    S = kernel_constant("kPnpMinSlice")
    rng = np.random.default_rng(21)
    cam = make_camera(rng, 40, bad_share=0.3)
    x, args, truth, bad = build([cam])
    set_problem(be, args)
    good, bads = np.flatnonzero(~bad), np.flatnonzero(bad)
    opts = dict(threshold=2.0)
    # the winner: the inlier triple the restatement scores highest; every other sample holds a displaced observation
    trials = [rng.choice(good, 3, replace=False) for _ in range(12)]
    scores = [pr.hypothesis(cam[0], cam[1], K, t, 2.0, 0.0) for t in trials]
    k = int(np.argmax([s["count"] for s in scores]))
    win, top = trials[k], scores[k]
    assert not top["close"] and top["count"] >= 0.8 * len(good)

    def losers(H):
        s = np.stack([rng.choice(good, 3, replace=False) for _ in range(H)])
        s[:, 0] = rng.choice(bads, H)
        return s.astype(np.int32)

    def slice_len(H):                                            # one camera: H // S slices (fewer only on a device of under H // 2S CUs)
        sl = max(1, H // S)
        return (H + sl - 1) // sl

    for H in (1, S - 1, S, S + 1, 2 * S - 1, 2 * S, 256, 257):
        samples = losers(H)
        hs = slice_len(H)
        for pos in sorted({0, H - 1, min(H - 1, hs - 1), min(H - 1, hs), min(H - 1, 2 * hs - 1), min(H - 1, 2 * hs), min(H - 1, 63), min(H - 1, 64)}):
            s = samples.copy()
            s[pos] = win
            res = be.resect_ransac(x, samples=s[None], want_hyp=True, **opts)
            assert res.hyp_inliers.shape == (1, H) and res.best[0] == pos and res.inliers[0] == top["count"], (H, pos)
            assert res.hyp_inliers[0, pos] == top["count"] and res.best_sol[0] == top["sol"] and res.status[0] == res.OK
            assert np.array_equal(res.inlier_mask, top["mask"])
    # equal counts: the lowest h, across waves and slices
    H = 257
    samples = losers(H)
    hs = slice_len(H)
    for pair in ((5, 6), (63, 64), (hs - 1, hs), (70, 200), (3, 256), (2 * hs - 1, 2 * hs + 1)):
        s = samples.copy()
        s[list(pair)] = win
        res = be.resect_ransac(x, samples=s[None], want_hyp=True, **opts)
        assert res.best[0] == min(pair) and res.hyp_inliers[0, pair[0]] == res.hyp_inliers[0, pair[1]] == top["count"], pair
    # every hypothesis of one such call against the restatement
    s = samples.copy()
    s[130] = win
    res = be.resect_ransac(x, samples=s[None], want_hyp=True, **opts)
    assert check_against(res, pr.resect_ransac(x, args, samples=s[None], **opts), args[2], "H = 257") == 1
    # an invalid sample counts -1 and never wins; only invalid samples: no best
    s[7] = [4, 4, 9]
    res = be.resect_ransac(x, samples=s[None], want_hyp=True, **opts)
    assert res.hyp_inliers[0, 7] == -1 and res.best[0] == 130
    res = be.resect_ransac(x, samples=np.tile(np.array([[1, 1, 2]], dtype=np.int32), (1, 5, 1)), want_hyp=True)
    assert np.all(res.hyp_inliers == -1) and res.best[0] == -1 and res.best_sol[0] == -1 and res.status[0] == res.DEGENERATE
    assert res.inliers[0] == 0 and not res.inlier_mask.any() and res.cameras[0].tobytes() == x[:6].tobytes()


# ---- batches -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C", [1, 2, 257])
def test_batches(be, C):
    rng = np.random.default_rng(100 + C)
    cams = [make_camera(rng, int(n), bad_share=0.25) for n in rng.integers(8, 14, C)]
    junk = rng.normal(0.0, 0.3, (C, 6))
    x, args, truth, bad = build(cams, x_cams=junk)
    ci = args[2]
    set_problem(be, args)
    sel = np.ones(C, dtype=bool)
    use = np.ones(len(ci), dtype=bool)
    if C > 1:
        sel[1] = False                                           # not selected
    if C > 2:
        sel[100] = False
        use[ci == 5] = False                                     # selected, no used observation
        use[ci == 200] = False
    opts = dict(max_iters=12, threshold=2.0, min_views=4, seed=C)
    res = be.resect_ransac(x, select=sel, obs_use=use, want_hyp=True, **opts)
    ref = pr.resect_ransac(x, args, select=sel, obs_use=use, **opts)
    n_sure = check_against(res, ref, ci, f"{C} cameras")
    print(f"{C} cameras: {n_sure} compared in full, {res.n_ok} OK")
    assert n_sure >= C // 2 and res.n_ok == int((res.status == 0).sum())
    off = ~sel
    assert np.all(res.status[off] == res.NOT_SELECTED) and res.cameras[off].tobytes() == junk[off].tobytes()
    assert res.hyp[off].tobytes() == junk[off].tobytes() and np.all(res.views[off] == 0) and not res.inlier_mask[off[ci]].any()
    assert np.all(res.hyp_inliers[off] == -1) and np.all(res.best[off] == -1) and np.isnan(res.rms_err[off]).all()
    if C > 2:
        for c in (5, 200):
            assert res.status[c] == res.FEW_VIEWS and res.views[c] == 0 and res.cameras[c].tobytes() == junk[c].tobytes()
    not_ok = res.status != res.OK
    assert res.cameras[not_ok].tobytes() == junk[not_ok].tobytes()
    assert not res.inlier_mask[~use].any()


# ---- every status, success, refine ---------------------------------------------------------------------------------------------

def test_every_status_success_and_refine(be):
    rng = np.random.default_rng(9)
    clean = make_camera(rng, 60, bad_share=0.2)
    few = make_camera(rng, 3, bad_share=0.0)
    noise = make_camera(rng, 40, bad_share=0.0)
    noise = (noise[0], rng.uniform(0.0, 2000.0, (40, 2)), noise[2], noise[3])     # pixels that fit no pose
    other = make_camera(rng, 20, bad_share=0.0)
    junk = rng.normal(0.0, 0.3, (4, 6))
    x, args, truth, bad = build([clean, few, noise, other], x_cams=junk)
    set_problem(be, args)
    sel = np.array([1, 1, 1, 0], dtype=bool)
    opts = dict(max_iters=64, threshold=2.0, seed=1)
    res = be.resect_ransac(x, select=sel, **opts)
    ref = pr.resect_ransac(x, args, select=sel, **opts)
    assert list(res.status) == [res.OK, res.FEW_VIEWS, res.DEGENERATE, res.NOT_SELECTED] == list(ref["status"])
    assert list(res.views) == [60, 3, 40, 0] and res.n_ok == 1
    assert res.cameras[1:].tobytes() == junk[1:].tobytes() and np.isnan(res.rms_err[1:]).all() and np.all(res.iters[1:] == 0)
    # DEGENERATE still reports its best hypothesis: count, h, solution, mask
    assert check_against(res, ref, args[2], "statuses") >= 3
    assert res.inliers[2] < 6 and res.best[2] >= 0 and res.inlier_mask[args[2] == 2].sum() == res.inliers[2]
    # HIGH_ERROR: 0.5 px of noise against an rms threshold of 0.1 px
    hi = be.resect_ransac(x, select=sel, max_rms_px=0.1, **opts)
    assert hi.status[0] == hi.HIGH_ERROR and hi.rms_err[0] > 0.1 and hi.cameras[0].tobytes() == junk[0].tobytes()
    assert hi.hyp[0].tobytes() == res.hyp[0].tobytes() and hi.inliers[0] == res.inliers[0]
    # success on both sides of confidence
    ratio = res.inliers[0] / 60.0
    assert be.resect_ransac(x, select=sel, confidence=ratio, **opts).success[0]
    assert not be.resect_ransac(x, select=sel, confidence=np.nextafter(ratio, 1.0), **opts).success[0]
    assert not res.success[0] and not res.success[1:].any()
    # refine = 0: the best hypothesis itself, its rms error over the inliers, no trial pose
    raw = be.resect_ransac(x, select=sel, refine=0, **opts)
    assert raw.status[0] == raw.OK and raw.cameras[0].tobytes() == raw.hyp[0].tobytes() == res.hyp[0].tobytes() and raw.iters[0] == 0
    Xc, uvc = clean[0][res.inlier_mask[:60]], clean[1][res.inlier_mask[:60]]
    assert abs(raw.rms_err[0] - np.sqrt(2.0 * rr.cost(raw.hyp[0], Xc, uvc, K) / len(Xc))) <= 1e-9 * raw.rms_err[0]
    assert res.iters[0] >= 1 and res.rms_err[0] <= raw.rms_err[0]
    d = rr.gauss_newton_step(res.cameras[0], Xc, uvc, K)
    assert np.sqrt(d @ d) <= 100.0 * XTOL * (np.linalg.norm(res.cameras[0]) + XTOL)
    # BEHIND: a depth threshold between the smallest inlier depth at the best hypothesis and at the refined pose
    found = False
    for seed in range(40):
        cam = make_camera(np.random.default_rng(500 + seed), 30, bad_share=0.2)
        xb, argsb, _, _ = build([cam])
        r0 = pr.resect_ransac(xb, argsb, **opts)
        if r0["status"][0] != pr.OK or r0["hyp_close"][0].any():
            continue
        m = r0["inlier_mask"]
        depth = lambda p: ((cam[0][m] - p[3:]) @ rr.orc.rodrigues(p[:3])[2]).min()
        lo, hi_d = depth(r0["cameras"][0]), depth(r0["hyp"][0])
        if hi_d - lo > 1e-6:
            found = True
            break
    assert found
    set_problem(be, argsb)
    mid = 0.5 * (lo + hi_d)
    rb = be.resect_ransac(xb, min_depth=mid, **opts)
    assert rb.status[0] == rb.BEHIND and rb.cameras[0].tobytes() == xb[:6].tobytes() and np.isfinite(rb.rms_err[0])
    assert np.array_equal(rb.inlier_mask, m) and be.resect_ransac(xb, min_depth=lo - 1e-6, **opts).status[0] == rb.OK


# ---- masks -----------------------------------------------------------------------------------------------------------------------

def test_masks(be, three):
    x, args, truth, bad = three
    C, P, ci, pi, uv, _ = args
    rng = np.random.default_rng(4)
    use = rng.permutation(len(ci)) >= len(ci) // 8
    opts = dict(max_iters=32, threshold=2.0, seed=9)
    set_problem(be, args)
    masked = be.resect_ransac(x, obs_use=use, want_hyp=True, **opts)
    # the problem without those observations (the points keep their numbers)
    set_problem(be, (C, P, ci[use], pi[use], uv[use], K))
    removed = be.resect_ransac(x, want_hyp=True, **opts)
    for name in FIELDS + ("hyp_inliers",):
        if name != "inlier_mask":
            assert getattr(masked, name).tobytes() == getattr(removed, name).tobytes(), name
    assert np.array_equal(masked.inlier_mask[use], removed.inlier_mask) and not masked.inlier_mask[~use].any()


def test_mask_of_exactly_the_displaced_observations_matches_plain_resection(be):
    rng = np.random.default_rng(44)
    cams = [make_camera(rng, n, noise=0.05) for n in (25, 50)]
    x, args, truth, bad = build(cams)
    set_problem(be, args)
    plain = be.resect(x, obs_use=~bad)
    rob = be.resect_ransac(x, obs_use=~bad, max_iters=32, seed=2)   # 0.05 px of noise against 8 px: every observation an inlier
    assert np.array_equal(rob.inlier_mask, ~bad) and np.all(rob.status == rob.OK)
    for c in range(2):
        assert near(rob.cameras[c], plain.cameras[c]), c


# ---- storage precision -------------------------------------------------------------------------------------------------------------

def test_fp32_storage_reads_the_rounded_pixels(be, three):
    x, args, truth, bad = three
    C, P, ci, pi, uv, _ = args
    rounded = uv.astype(np.float32).astype(np.float64)
    opts = dict(max_iters=32, threshold=2.0, seed=3)
    try:
        set_problem(be, args, bits=32)
        res = be.resect_ransac(x, want_hyp=True, **opts)
    finally:
        be.set_precision(64)
    assert check_against(res, pr.resect_ransac(x, (C, P, ci, pi, rounded, K), **opts), ci, "fp32") >= 2
    for c in range(C):
        m = res.inlier_mask & (ci == c)
        X = x[6 * C:].reshape(P, 3)[pi[m]]
        rms_r = np.sqrt(2.0 * rr.cost(res.cameras[c], X, rounded[m], K) / m.sum())
        rms_u = np.sqrt(2.0 * rr.cost(res.cameras[c], X, uv[m], K) / m.sum())
        assert abs(res.rms_err[c] - rms_r) <= 1e-11 * rms_r and abs(res.rms_err[c] - rms_u) > 1e-9 * rms_u


# ---- determinism -----------------------------------------------------------------------------------------------------------------

def test_same_bits_twice_and_in_another_observation_order(be):
    """Three cameras that share points; camera 1 sees point 3 twice."""
    rng = np.random.default_rng(41)
    P = 120
    pts = np.stack([rng.uniform(-2, 2, P), rng.uniform(-1.5, 1.5, P), rng.uniform(5.0, 9.0, P)], axis=1)
    truth = np.array([[0.02, -0.1, 0.03, -0.6, 0.1, 0.0], [-0.05, 0.12, 0.2, 0.5, -0.2, 0.3], [0.1, 0.3, -0.1, 1.0, 0.2, -0.4]])
    ci, pi = [], []
    for c in range(3):
        seen = np.sort(rng.choice(P, 80, replace=False))
        if c == 1:
            seen = np.sort(np.append(seen[seen != 3], [3, 3]))
        ci.append(np.full(len(seen), c)); pi.append(seen)
    ci, pi = np.concatenate(ci).astype(np.int64), np.concatenate(pi).astype(np.int64)
    x = np.concatenate([truth.ravel(), pts.ravel()])
    uv = rr.orc.compute_residuals(x, 3, P, ci, pi, np.zeros((len(ci), 2)), K).reshape(-1, 2) + rng.normal(0.0, 0.3, (len(ci), 2))
    wrong = rng.random(len(ci)) < 0.25
    uv[wrong] += rng.uniform(30.0, 120.0, (int(wrong.sum()), 2))
    use = rng.permutation(len(ci)) >= len(ci) // 10
    opts = dict(max_iters=40, threshold=2.0, seed=7)
    set_problem(be, (3, P, ci, pi, uv, K))
    first, again = be.resect_ransac(x, want_hyp=True, **opts), be.resect_ransac(x, want_hyp=True, **opts)
    masked = be.resect_ransac(x, obs_use=use, want_hyp=True, **opts)
    assert np.all(first.status == first.OK) and not np.any(first.inlier_mask & wrong)
    for name in FIELDS + ("hyp_inliers",):
        assert getattr(first, name).tobytes() == getattr(again, name).tobytes(), name
    key = np.random.default_rng(6).permutation(3 * P)[ci * P + pi]
    perm = np.argsort(key, kind="stable")                        # shuffled, a repeated pair keeps its order
    assert np.any(np.diff(pi[perm]) < 0) and np.any(np.diff(ci[perm]) < 0)
    set_problem(be, (3, P, ci[perm], pi[perm], uv[perm], K))
    sh, shm = be.resect_ransac(x, want_hyp=True, **opts), be.resect_ransac(x, obs_use=use[perm], want_hyp=True, **opts)
    for name in FIELDS + ("hyp_inliers",):
        a, b = (getattr(first, name), getattr(masked, name))
        if name == "inlier_mask":
            a, b = a[perm], b[perm]
        assert getattr(sh, name).tobytes() == a.tobytes(), name
        assert getattr(shm, name).tobytes() == b.tobytes(), name


# ---- isolation, errors, timing -------------------------------------------------------------------------------------------------

def test_robust_resection_does_not_disturb_a_solve():
    import sfmba
    pb = sfmba.make_problem(8, 120, 900, seed=21)
    use = np.arange(pb.n_obs) % 3 != 0

    def solve(b, before=False, between=False):
        b.set_precision(64)
        b.set_problem(*pb.args)
        if before:
            b.resect_ransac(pb.x_true, obs_use=use, max_iters=32)
        opt = b.default_options()
        opt.ftol = 1e-10
        xs, res, _, _ = b.solve(pb.x0, opt, want_fun=False, want_grad=False)     # fun, grad stay on the device
        if between:
            kept = b.fetch_fun_grad()
            b.resect_ransac(pb.x0, select=np.arange(8) % 2 == 0, max_iters=32)   # at ANOTHER x than the solve's result
            after = b.fetch_fun_grad()
            assert kept[0].tobytes() == after[0].tobytes() and kept[1].tobytes() == after[1].tobytes()
        fun, grad = b.fetch_fun_grad()
        return xs, res.cost, int(res.nfev), fun, grad, b.pcg_history()

    results = []
    for kw in (dict(), dict(between=True), dict(before=True)):
        b = sfmba.Backend(0)
        try:
            results.append(solve(b, **kw))
        finally:
            b.close()
    want = results[0]
    for got in results[1:]:
        assert got[0].tobytes() == want[0].tobytes() and got[1] == want[1] and got[2] == want[2]
        assert got[3].tobytes() == want[3].tobytes() and got[4].tobytes() == want[4].tobytes() and got[5] == want[5]


def test_errors_and_timing(be, three):
    import sfmba
    x, args, truth, bad = three
    empty = sfmba.Backend(0)
    try:
        with pytest.raises(ValueError):
            empty.resect_ransac(np.zeros(0))
    finally:
        empty.close()
    set_problem(be, args)
    for kw in (dict(threshold=np.nan), dict(confidence=np.nan), dict(min_depth=np.nan), dict(xtol=np.nan), dict(max_rms_px=np.nan),
               dict(max_iters=0)):
        with pytest.raises(ValueError):
            be.resect_ransac(x, **kw)
    with pytest.raises(TypeError):
        be.resect_ransac(x, iterations=3)
    with pytest.raises(ValueError):
        be.resect_ransac(x, select=np.ones(4, dtype=bool))
    with pytest.raises(ValueError):
        be.resect_ransac(x, samples=np.zeros((3, 4, 8), dtype=np.int32))
    s = np.tile(np.array([0, 1, 2], dtype=np.int32), (3, 4, 1))
    assert be.resect_ransac(x, samples=s).status.shape == (3,)
    for wrong in (-1, 30):                                       # camera 0 has 30 used observations: positions 0 .. 29
        t = s.copy()
        t[0, 2, 1] = wrong
        with pytest.raises(ValueError):
            be.resect_ransac(x, samples=t)
    t = s.copy()
    t[0, 2, 1] = 29
    be.resect_ransac(x, samples=t)
    # the handle still works after a refused call, and only what is asked for is computed
    ok = be.resect_ransac(x, max_iters=8, profile=1)
    assert ok.hyp_inliers is None and ok.kernel_us > 0.0 and be.resect_ransac(x, max_iters=8).kernel_us == 0.0
    assert be.time_kernel(x, 17, 2) > 0.0
