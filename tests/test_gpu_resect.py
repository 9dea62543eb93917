"""GPU tests of sfmba_resect (k_resect): the linear stage and the final pose against the reference's recorded output, the
refinement against the oracle's Gauss-Newton step, run lengths at the loop's edges, every status, rotations at the branch
points of the rotation vector, masks, bitwise repeatability, storage precision, isolation from the solver and the timing
entry.

Bounds.  Against the reference: the numpy restatement's own distance to it, times 100, recorded by
tools/gen_resect_golden.py in tests/golden/resect_bounds.json.  Refinement: at the returned pose the oracle's next
Gauss-Newton step is at most 100 xtol (|p| + xtol) -- one contraction of the iteration plus the difference between the
oracle's and the kernel's Jacobian; two results that both satisfy it lie within 200 xtol (|p| + xtol) of each other."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

import resect_ref as rr
from kernel_source import kernel_constant

pytestmark = pytest.mark.gpu

XTOL = 1e-10
BOUNDS = json.load(open(os.path.join(GOLDEN, "resect_bounds.json")))
K = np.array([[2905.88, 0.0, 1416.0], [0.0, 2905.88, 1064.0], [0.0, 0.0, 1.0]])
FIELDS = ("cameras", "status", "views", "iters", "rms_err")


@pytest.fixture(scope="module")
def be():
    import sfmba
    b = sfmba.Backend(0)
    yield b
    b.close()


def make_camera(rng, n, noise, w=None, T=None, coplanar=False):
    """A pose and n points 4..9 units in front of it with their pixels -> (X (n, 3), uv (n, 2), params (6))."""
    if w is None:
        w = rng.normal(size=3)
        w *= rng.uniform(0.2, 1.0) / np.linalg.norm(w)
    w = np.asarray(w, dtype=np.float64)
    T = rng.normal(0.0, 1.5, 3) if T is None else np.asarray(T, dtype=np.float64)
    R = rr.orc.rodrigues(w)
    cam = np.stack([rng.uniform(-1.8, 1.8, n), rng.uniform(-1.3, 1.3, n),
                    np.full(n, 6.0) if coplanar else rng.uniform(4.0, 9.0, n)], axis=1)
    uv = cam @ K.T
    uv = uv[:, :2] / uv[:, 2:3] + noise * rng.normal(size=(n, 2))
    return cam @ R + T, uv, np.concatenate([w, T])


def build(cams, x_cams=None):
    """One problem of the cameras' own points -> (x, args, truth (C, 6)); the cameras of x are `x_cams` (default: truth)."""
    C = len(cams)
    n = [len(c[0]) for c in cams]
    ci = np.repeat(np.arange(C, dtype=np.int64), n)
    pi = np.arange(sum(n), dtype=np.int64)
    X = np.concatenate([c[0] for c in cams]).reshape(-1, 3)
    uv = np.concatenate([c[1] for c in cams]).reshape(-1, 2)
    truth = np.stack([c[2] for c in cams])
    x = np.concatenate([(truth if x_cams is None else x_cams).ravel(), X.ravel()])
    return x, (C, len(pi), ci, pi, uv, K), truth


def camera_data(x, args, c, obs_use=None):
    """(X, uv) of camera c in camera-major stored order."""
    C, P, ci, pi, uv, _ = args
    idx = rr.camera_slices(ci, pi, C)[c]
    if obs_use is not None:
        idx = idx[np.asarray(obs_use).astype(bool)[idx]]
    return x[6 * C:].reshape(P, 3)[pi[idx]], np.asarray(uv, dtype=np.float64)[idx]


def next_step_ratio(p, X, uv):
    d = rr.gauss_newton_step(p, X, uv, K)
    return float(np.sqrt(d @ d) / (XTOL * (np.sqrt(p @ p) + XTOL)))


def near(p, q, factor=200.0):
    return float(np.sqrt(((p - q) ** 2).sum())) <= factor * XTOL * (np.sqrt(q @ q) + XTOL)


def pose_distance(p, R_ref, T_ref):
    return rr.rotation_angle(R_ref, rr.orc.rodrigues(p[:3])), float(np.linalg.norm(p[3:] - T_ref))


def set_problem(be, args, bits=64):
    be.set_precision(bits)
    be.set_fixed_cameras(())
    be.set_problem(*args)


# ---- test 1: the fixture cases through solve_pnp ------------------------------------------------------------------------------

def test_fixture_cases_through_solve_pnp(be):
    import sfmba
    g = np.load(os.path.join(GOLDEN, "resect_cases.npz"), allow_pickle=False)
    worst = dict(linear_R_angle=0.0, final_R_angle=0.0, final_T_dist=0.0)
    for k in range(len(g["n"])):
        sl = slice(int(g["ptr"][k]), int(g["ptr"][k + 1]))
        X, uv = g["X"][sl], g["uv"][sl]
        ok, rvec, tvec = sfmba.solve_pnp(X, uv, g["K"], backend=be, max_iter=0)
        assert ok and rvec.shape == (3, 1) and tvec.shape == (3, 1)
        a_lin = rr.rotation_angle(g["R_lin"][k], rr.orc.rodrigues(rvec.ravel()))
        ok, rvec, tvec = sfmba.solve_pnp(X, uv, g["K"], None, backend=be)
        assert ok
        R, R_ref = rr.orc.rodrigues(rvec.ravel()), rr.orc.rodrigues(g["rvec"][k])
        a_fin = rr.rotation_angle(R_ref, R)
        d_fin = float(np.linalg.norm(-R.T @ tvec.ravel() + R_ref.T @ g["tvec"][k]))
        print(f"n={int(g['n'][k])} noise={float(g['noise'][k])}: linear R {a_lin:.2e}, final R {a_fin:.2e}, T {d_fin:.2e}")
        for key, val in (("linear_R_angle", a_lin), ("final_R_angle", a_fin), ("final_T_dist", d_fin)):
            worst[key] = max(worst[key], val)
            assert val <= BOUNDS[key]["bound"], (k, key, val)
        if g["noise"][k] == 0.0:                                 # exact data: the generating pose
            R_true = rr.orc.rodrigues(g["rvec_true"][k])
            assert rr.rotation_angle(R_true, R) <= BOUNDS["final_R_angle"]["bound"]
            assert np.linalg.norm(-R.T @ tvec.ravel() + R_true.T @ g["tvec_true"][k]) <= BOUNDS["final_T_dist"]["bound"]
    for key, val in worst.items():
        print(f"{key}: {val:.3e} (restatement {BOUNDS[key]['measured_max']:.3e}, bound {BOUNDS[key]['bound']:.3e})")


# ---- test 2: the refinement ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def four():
    rng = np.random.default_rng(31)
    cams = [make_camera(rng, n, 0.5) for n in (40, 90, 150, 300)]
    return build(cams)


def test_refinement_reaches_the_gauss_newton_fixed_point(be, four):
    x, args, truth = four
    C = args[0]
    set_problem(be, args)
    lin = be.resect(x, max_iter=0)
    res = be.resect(x)
    assert np.all(lin.status == lin.OK) and np.all(res.status == res.OK) and np.all(lin.iters == 0)
    assert res.n_ok == C and np.array_equal(res.ok, res.status == 0) and res.iters.max() <= 8 and res.iters.min() >= 1
    xp = x.copy()
    xp[:6 * C] += np.random.default_rng(2).normal(0.0, 5e-3, 6 * C)
    pose = be.resect(xp, start=1)
    assert np.all(pose.status == pose.OK)
    r = be.residuals(np.concatenate([res.cameras.ravel(), x[6 * C:]])).reshape(-1, 2)
    for c in range(C):
        X, uv = camera_data(x, args, c)
        ratio = next_step_ratio(res.cameras[c], X, uv)
        print(f"camera {c}: next step / (xtol (|p| + xtol)) = {ratio:.3g} (bound 100), {int(res.iters[c])} trial poses; "
              f"pose-only from a perturbed pose: {next_step_ratio(pose.cameras[c], X, uv):.3g}, {int(pose.iters[c])}")
        assert ratio <= 100.0 and next_step_ratio(pose.cameras[c], X, uv) <= 100.0
        # (1e-13: the oracle adds the cost up in another order than the kernel that took the decisions)
        assert rr.cost(res.cameras[c], X, uv, K) <= rr.cost(lin.cameras[c], X, uv, K) * (1.0 + 1e-13)
        assert rr.cost(pose.cameras[c], X, uv, K) <= rr.cost(xp[6 * c:6 * c + 6], X, uv, K) * (1.0 + 1e-13)
        assert near(pose.cameras[c], res.cameras[c])
        e2 = (r[args[2] == c] ** 2).sum()
        assert abs(res.rms_err[c] - np.sqrt(e2 / res.views[c])) <= 1e-12 * res.rms_err[c]
        assert 0.3 < res.rms_err[c] < 1.0                        # 0.5 px of noise per coordinate
    ref = rr.resect(x, args)
    assert np.array_equal(ref["status"], res.status) and all(near(res.cameras[c], ref["cameras"][c]) for c in range(C))


# ---- test 3: run lengths at the loop's edges ----------------------------------------------------------------------------------

def test_run_lengths_at_the_edges_of_the_loop(be):
    """Cameras with 0, 5, 6, 7, 255, 256, 257 and 256 unroll -+ 1 observations in one problem (nine cameras, 2834
    observations: the list of run lengths decides the size)."""
    T, U = kernel_constant("kCamThreads"), kernel_constant("kResectUnroll")
    assert T == 256 and U >= 2
    lengths = [0, 5, 6, 7, T - 1, T, T + 1, T * U - 1, T * U + 1]
    rng = np.random.default_rng(77)
    x, args, truth = build([make_camera(rng, n, 0.5) for n in lengths], x_cams=np.full((len(lengths), 6), 0.25))
    set_problem(be, args)
    res = be.resect(x)
    lin = be.resect(x, max_iter=0)
    ref = rr.resect(x, args)
    ref_lin = rr.resect(x, args, max_iter=0)
    assert np.array_equal(res.views, lengths) and np.array_equal(lin.views, lengths)
    assert np.array_equal(res.status, ref["status"]) and np.array_equal(lin.status, ref_lin["status"])
    assert np.array_equal(res.status[:2], [res.FEW_VIEWS] * 2) and np.all(res.status[2:] == res.OK)
    assert res.cameras[:2].tobytes() == x[:12].tobytes() and np.all(np.isnan(res.rms_err[:2])) and np.all(res.iters[:2] == 0)
    assert res.n_ok == len(lengths) - 2
    for c in range(2, len(lengths)):
        X, uv = camera_data(x, args, c)
        # the linear stage: as far from the restatement's as the restatement is from the reference, times 100
        a = rr.rotation_angle(rr.orc.rodrigues(ref_lin["cameras"][c, :3]), rr.orc.rodrigues(lin.cameras[c, :3]))
        print(f"n={lengths[c]}: linear R vs restatement {a:.2e} rad; final pose next step ratio {next_step_ratio(res.cameras[c], X, uv):.3g}")
        assert a <= BOUNDS["linear_R_angle"]["bound"]
        assert near(res.cameras[c], ref["cameras"][c]) and next_step_ratio(res.cameras[c], X, uv) <= 100.0


# ---- test 4: every status -------------------------------------------------------------------------------------------------------

def test_every_status_and_pass_through(be):
    rng = np.random.default_rng(5)
    exact = make_camera(rng, 40, 0.0)
    noisy = make_camera(rng, 60, 0.5)
    flat = make_camera(rng, 50, 0.0, coplanar=True)
    # exact data plus one correspondence whose point lies BEHIND the generating pose (its pixel is still its projection)
    Xb, uvb, pb = make_camera(rng, 30, 0.0)
    Rb = rr.orc.rodrigues(pb[:3])
    back = np.array([0.4, -0.3, -5.0])
    pix = K @ back
    behind = (np.vstack([Xb, back @ Rb + pb[3:]]), np.vstack([uvb, pix[:2] / pix[2]]), pb)
    few = make_camera(rng, 5, 0.0)
    other = make_camera(rng, 20, 0.0)
    junk = rng.normal(0.0, 0.3, (6, 6))
    x, args, truth = build([exact, noisy, flat, behind, few, other], x_cams=junk)
    set_problem(be, args)
    sel = np.array([1, 1, 1, 1, 1, 0], dtype=bool)
    res = be.resect(x, select=sel)
    assert list(res.status) == [res.OK, res.OK, res.DEGENERATE, res.BEHIND, res.FEW_VIEWS, res.NOT_SELECTED]
    assert list(res.views) == [40, 60, 50, 31, 5, 0]
    assert res.n_ok == int((res.status == 0).sum()) == 2
    bad = res.status != 0
    assert res.cameras[bad].tobytes() == junk[bad].tobytes()
    assert np.isfinite(res.rms_err[3]) and res.rms_err[3] < 1e-6 and np.isnan(res.rms_err[[2, 4, 5]]).all()
    for c in (0, 1):
        X, uv = camera_data(x, args, c)
        assert next_step_ratio(res.cameras[c], X, uv) <= 100.0
    a, d = pose_distance(res.cameras[0], rr.orc.rodrigues(truth[0, :3]), truth[0, 3:])
    assert a <= BOUNDS["final_R_angle"]["bound"] and d <= BOUNDS["final_T_dist"]["bound"]
    # without the depth test the camera with the point behind it is the generating pose
    nb = be.resect(x, select=sel, min_depth=-np.inf)
    assert nb.status[3] == nb.OK
    a, d = pose_distance(nb.cameras[3], Rb, pb[3:])
    assert a <= BOUNDS["final_R_angle"]["bound"] and d <= BOUNDS["final_T_dist"]["bound"]
    # an rms threshold between the exact cameras' error and the noisy camera's
    hi = be.resect(x, max_rms_px=0.1, min_depth=-np.inf)
    assert list(hi.status) == [hi.OK, hi.HIGH_ERROR, hi.DEGENERATE, hi.OK, hi.FEW_VIEWS, hi.OK]
    assert hi.rms_err[1] > 0.1 and hi.cameras[1].tobytes() == junk[1].tobytes() and hi.n_ok == 3
    # from the pose in x the plane is no obstacle, and three views are enough
    xs = x.copy()
    xs[:36] = (truth + rng.normal(0.0, 2e-3, truth.shape)).ravel()
    st = be.resect(xs, start=1, min_depth=-np.inf, min_views=0)
    assert np.all(st.status == st.OK) and list(st.views) == [40, 60, 50, 31, 5, 20]
    for c in range(6):
        X, uv = camera_data(xs, args, c)
        assert next_step_ratio(st.cameras[c], X, uv) <= 100.0, c
        if c != 1:                                               # exact data: the minimiser is the generating pose
            assert near(st.cameras[c], truth[c]), c
    # the restatement takes the same decisions
    ref = rr.resect(x, args, select=sel)
    assert np.array_equal(ref["status"], res.status) and np.array_equal(ref["views"], res.views)


# ---- test 5: rotations at the branch points ---------------------------------------------------------------------------------------

def test_rotations_at_the_branch_points(be):
    rng = np.random.default_rng(12)
    axis = np.array([0.6, -0.48, 0.64])
    ws = [np.zeros(3), axis * (np.pi - 5e-4), -axis * (np.pi - 2e-4), axis * 1e-9,
          np.array([np.pi - 1e-4, 0.0, 0.0]), np.array([0.0, 0.0, np.pi - 1e-4])]
    cams = [make_camera(rng, 30, 0.0, w=w) for w in ws]
    x, args, truth = build(cams, x_cams=np.zeros((len(ws), 6)))
    set_problem(be, args)
    for kw in (dict(max_iter=0), dict()):
        res = be.resect(x, **kw)
        assert np.all(res.status == res.OK)
        for c, w in enumerate(ws):
            a, d = pose_distance(res.cameras[c], rr.orc.rodrigues(w), truth[c, 3:])
            print(f"|w| = {np.linalg.norm(w):.9g} {kw}: R off by {a:.2e} rad, T by {d:.2e}")
            assert a <= BOUNDS["final_R_angle"]["bound"] and d <= BOUNDS["final_T_dist"]["bound"]
            assert np.linalg.norm(res.cameras[c, :3]) <= np.pi * (1 + 1e-12)


# ---- tests 6 and 7: masks, a repeated pair, same bits ----------------------------------------------------------------------------

@pytest.fixture(scope="module")
def shared():
    """Three cameras that share points; camera 1 sees point 3 twice (two pixels 0.4 px apart)."""
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
    use = rng.permutation(len(ci)) >= len(ci) // 10              # drops a tenth
    return x, (3, P, ci, pi, uv, K), use


def test_repeated_pair_and_observation_mask(be, shared):
    x, args, use = shared
    C, P, ci, pi, uv, _ = args
    assert ((ci == 1) & (pi == 3)).sum() == 2 and (~use).sum() == len(ci) // 10
    set_problem(be, args)
    for mask in (None, use):
        res = be.resect(x, obs_use=mask)
        ref = rr.resect(x, args, obs_use=mask)
        assert np.all(res.status == res.OK) and np.array_equal(res.views, ref["views"])
        assert np.array_equal(res.views, np.bincount(ci, weights=None if mask is None else mask.astype(float)).astype(int))
        for c in range(C):
            X, uvc = camera_data(x, args, c, mask)
            assert len(X) == res.views[c] and next_step_ratio(res.cameras[c], X, uvc) <= 100.0
            assert near(res.cameras[c], ref["cameras"][c])
    assert not near(be.resect(x, obs_use=use).cameras[1], be.resect(x).cameras[1], factor=2.0)   # the mask is read


def test_same_bits_twice_and_in_another_observation_order(be, shared):
    x, args, use = shared
    C, P, ci, pi, uv, _ = args
    set_problem(be, args)
    first, again = be.resect(x), be.resect(x)
    masked = be.resect(x, obs_use=use)
    for name in FIELDS:
        assert getattr(first, name).tobytes() == getattr(again, name).tobytes(), name
    # shuffled by a key per (camera, point) pair, stable: a repeated pair keeps its order
    key = np.random.default_rng(6).permutation(C * P)[ci * P + pi]
    perm = np.argsort(key, kind="stable")
    assert np.any(np.diff(pi[perm]) < 0) and np.any(np.diff(ci[perm]) < 0)
    set_problem(be, (C, P, ci[perm], pi[perm], uv[perm], K))
    sh, shm = be.resect(x), be.resect(x, obs_use=use[perm])
    for name in FIELDS:
        assert getattr(sh, name).tobytes() == getattr(first, name).tobytes(), name
        assert getattr(shm, name).tobytes() == getattr(masked, name).tobytes(), name


# ---- test 8: storage precision ------------------------------------------------------------------------------------------------------

def test_fp32_storage_reads_the_rounded_pixels(be, four):
    x, args, truth = four
    C, P, ci, pi, uv, _ = args
    rounded = uv.astype(np.float32).astype(np.float64)
    assert np.abs(rounded - uv).max() > 1e-5
    try:
        set_problem(be, args, bits=32)
        res, lin = be.resect(x), be.resect(x, max_iter=0)
    finally:
        be.set_precision(64)
    ref = rr.resect(x, (C, P, ci, pi, rounded, K))
    ref_lin = rr.resect(x, (C, P, ci, pi, rounded, K), max_iter=0)
    assert np.all(res.status == res.OK)
    for c in range(C):
        X, uvc = camera_data(x, (C, P, ci, pi, rounded, K), c)
        assert near(res.cameras[c], ref["cameras"][c]) and next_step_ratio(res.cameras[c], X, uvc) <= 100.0
        a = rr.rotation_angle(rr.orc.rodrigues(ref_lin["cameras"][c, :3]), rr.orc.rodrigues(lin.cameras[c, :3]))
        assert a <= BOUNDS["linear_R_angle"]["bound"]
        # the error is that of the rounded pixels, not of the unrounded ones
        X0, uv0 = camera_data(x, args, c)
        rms_r = np.sqrt(2.0 * rr.cost(res.cameras[c], X, uvc, K) / len(X))
        rms_u = np.sqrt(2.0 * rr.cost(res.cameras[c], X0, uv0, K) / len(X))
        assert abs(res.rms_err[c] - rms_r) <= 1e-11 * rms_r and abs(res.rms_err[c] - rms_u) > 1e-9 * rms_u


# ---- test 9: isolation, errors ------------------------------------------------------------------------------------------------------

def test_resection_does_not_disturb_a_solve():
    import sfmba
    pb = sfmba.make_problem(8, 120, 900, seed=21)
    use = np.arange(pb.n_obs) % 3 != 0

    def solve(b, before=False, between=False):
        b.set_precision(64)
        b.set_problem(*pb.args)
        if before:
            b.resect(pb.x_true, obs_use=use, max_rms_px=3.0)
        opt = b.default_options()
        opt.ftol = 1e-10
        xs, res, _, _ = b.solve(pb.x0, opt, want_fun=False, want_grad=False)     # fun, grad stay on the device
        if between:
            kept = b.fetch_fun_grad()
            b.resect(pb.x0, select=np.arange(8) % 2 == 0, start=1)             # at ANOTHER x than the solve's result
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


def test_errors_wrapper_and_timing(be, four):
    import sfmba
    x, args, truth = four
    empty = sfmba.Backend(0)
    try:
        with pytest.raises(ValueError):
            empty.resect(np.zeros(0))
    finally:
        empty.close()
    set_problem(be, args)
    for kw in (dict(xtol=np.nan), dict(min_depth=np.nan), dict(max_rms_px=np.nan)):
        with pytest.raises(ValueError):
            be.resect(x, **kw)
    with pytest.raises(TypeError):
        be.resect(x, max_iterations=3)
    with pytest.raises(ValueError):
        be.resect(x, select=np.ones(args[0] + 1, dtype=bool))
    with pytest.raises(ValueError):
        be.resect(x, obs_use=np.ones(len(args[2]) - 1, dtype=bool))
    # the args-tuple wrapper is the same call
    a = sfmba.resect_cameras(x, args, backend=be, max_iter=3)
    b = be.resect(x, max_iter=3)
    for name in FIELDS:
        assert getattr(a, name).tobytes() == getattr(b, name).tobytes(), name
    assert a.n_ok == b.n_ok
    # test 10: the timing entry
    assert be.time_kernel(x, 16, 2) > 0.0
