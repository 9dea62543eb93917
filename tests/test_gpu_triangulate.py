"""GPU tests of sfmba_triangulate (k_triangulate): the linear stage against the reference's recorded output and the SVD of
the same rows, the refinement against the oracle's Gauss-Newton step, every status, both run-handling forms, storage
precision and isolation from the solver, and `refine_reconstruction(retriangulate=True)`.

Bounds.  Linear stage: the numpy restatement's own distance to the reference, times 100 (fused multiply-adds, the Jacobi
rotation order and summation order), recorded by tools/gen_golden.py in tests/golden/triangulate_bounds.json.  Refinement:
at the returned point the next Gauss-Newton step is at most 100 xtol (|X| + xtol) -- one contraction of the iteration plus
the difference between the oracle's and the kernel's Jacobian."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

import consumer_inputs
import triangulate_ref as tr
from kernel_source import kernel_constant

pytestmark = pytest.mark.gpu

XTOL = 1e-10
BOUNDS = json.load(open(os.path.join(GOLDEN, "triangulate_bounds.json")))
LIN_REL = BOUNDS["problem"]["bound_rel"]


@pytest.fixture(scope="module")
def be():
    import sfmba
    b = sfmba.Backend(0)
    yield b
    b.close()


class Tracks:
    """Per-track numpy facts of a problem at x, computed once: runs in stored order, the SVD point of the DLT rows of
    the used observations, and the widest ray angle there."""

    def __init__(self, x, args, obs_use=None):
        C, P, ci, pi, uv, K = args
        self.x, self.args = np.asarray(x, dtype=np.float64), args
        self.C, self.P = C, P
        self.ci, self.pi, self.uv = np.asarray(ci).ravel(), np.asarray(pi).ravel(), np.asarray(uv, dtype=np.float64)
        self.K = K
        self.cams = self.x[:6 * C].reshape(C, 6)
        order, ptr = tr.stored_runs(self.pi, P)
        use = np.ones(len(self.ci), dtype=bool) if obs_use is None else np.asarray(obs_use).astype(bool)
        self.runs = [order[ptr[p]:ptr[p + 1]][use[order[ptr[p]:ptr[p + 1]]]] for p in range(P)]
        self.views = np.array([len(r) for r in self.runs])
        M = tr.projection_matrices(self.x, C, K)
        self.svd = np.full((P, 3), np.nan)
        self.angle = np.zeros(P)
        for p in np.flatnonzero(self.views >= 2):
            idx = self.runs[p]
            with np.errstate(all="ignore"):
                self.svd[p] = tr.svd_point(tr.dlt_rows(M[self.ci[idx]], self.uv[idx]))
                self.angle[p] = tr.widest_angle_deg(self.svd[p], self.cams[self.ci[idx], 3:])

    def next_step_ratio(self, p, X):
        """|next Gauss-Newton step| / (xtol (|X| + xtol)) at X, by the oracle."""
        idx = self.runs[p]
        d = tr.gauss_newton_step(X, self.cams, self.ci[idx], self.uv[idx], self.K)
        return float(np.sqrt(d @ d) / (XTOL * (np.sqrt(X @ X) + XTOL)))

    def cost(self, p, X):
        idx = self.runs[p]
        return tr.cost(X, self.cams, self.ci[idx], self.uv[idx], self.K)


def _check_linear(tk, points, which, bound=LIN_REL):
    """Test 1's comparison: the linear points against the SVD of the same rows, relative to max(1, |X|_inf)."""
    worst = 0.0
    for p in which:
        worst = max(worst, float(np.abs(points[p] - tk.svd[p]).max() / max(1.0, np.abs(tk.svd[p]).max())))
    print(f"linear stage vs SVD over {len(which)} tracks: {worst:.3e} (bound {bound:.3e})")
    assert worst <= bound
    return worst


def _check_refined(tk, tri, lin_points, which):
    """Test 2's assertions for the tracks `which` of a default-option result `tri`; `lin_points` their linear points."""
    ratios = [tk.next_step_ratio(p, tri.points[p]) for p in which]
    print(f"refinement over {len(which)} tracks: next step / (xtol (|X| + xtol)) up to {max(ratios):.3g} (bound 100), "
          f"iterations up to {int(tri.iters[which].max())}")
    assert max(ratios) <= 100.0
    assert tri.iters[which].max() <= 6
    for p in which:
        # (1e-13: the oracle adds the cost up in another order than the kernel that took the decisions)
        assert tk.cost(p, tri.points[p]) <= tk.cost(p, lin_points[p]) * (1.0 + 1e-13), p


def _run_rms(be, tk, tri, which):
    """rms of Backend.residuals over each run at the returned points."""
    x = np.concatenate([tk.x[:6 * tk.C], tri.points.ravel()])
    r = be.residuals(x).reshape(-1, 2)
    e2 = (r * r).sum(axis=1)
    return np.array([np.sqrt(e2[tk.runs[p]].sum() / len(tk.runs[p])) for p in which])


@pytest.fixture(scope="module")
def problem():
    import sfmba
    pb = sfmba.make_problem(6, 300, 1500, seed=3)
    tk = Tracks(pb.x_true, pb.args)
    two = np.flatnonzero(tk.views >= 2)
    cmp_ = np.flatnonzero((tk.views >= 2) & (tk.angle >= 2.0))
    assert len(two) == BOUNDS["problem"]["tracks_two_views"] and len(cmp_) == BOUNDS["problem"]["tracks_compared"]
    assert np.abs(tk.angle[two] - 2.0).min() > 1e-6 and np.abs(tk.angle[two] - 1.0).min() > 1e-6    # no verdict at rounding level
    return pb, tk, two, cmp_


# ---- test 1: the linear stage -------------------------------------------------------------------------------------------

def test_linear_stage_matches_the_reference_on_the_fixture(be):
    import sfmba
    g = np.load(os.path.join(GOLDEN, "triangulate_cases.npz"), allow_pickle=False)
    X = sfmba.triangulate_points(g["M1"], g["M2"], g["pts1"], g["pts2"], g["K"], backend=be)
    assert X.shape == g["X_ref"].shape and np.array_equal(X[3], np.ones(X.shape[1]))
    d = float(np.abs(X - g["X_ref"]).max())
    print(f"triangulate_points vs the reference: {d:.3e} (restatement {BOUNDS['fixture']['measured_abs']:.3e}, "
          f"bound {BOUNDS['fixture']['bound_abs']:.3e})")
    assert d <= BOUNDS["fixture"]["bound_abs"]


def test_linear_stage_matches_the_svd_on_the_problem(be, problem):
    pb, tk, two, cmp_ = problem
    be.set_precision(64)
    be.set_problem(*pb.args)
    assert len(cmp_) >= 0.95 * len(two)
    # the threshold that defines the compared set as the call's own, no depth test: every track left out says why
    tri = be.triangulate(pb.x_true, max_iter=0, min_angle_deg=2.0, min_depth=-np.inf)
    assert np.all(tri.status[cmp_] == tri.OK) and np.all(tri.iters == 0)
    _check_linear(tk, tri.points, cmp_)
    left = np.setdiff1d(np.arange(tk.P), cmp_)
    assert np.all(np.isin(tri.status[left], (tri.LOW_ANGLE, tri.FEW_VIEWS)))
    assert np.array_equal(tri.status[tk.views < 2], np.full(int((tk.views < 2).sum()), tri.FEW_VIEWS))
    assert np.array_equal(tri.views, tk.views)
    assert np.abs(tri.angle_deg[two] - tk.angle[two]).max() <= 1e-9
    # under the defaults (min_angle_deg = 1, min_depth = 0; first match wins) a track left out is short, narrow, behind a
    # camera -- the DLT of a one-camera track lands next to the camera centre -- or opens between 1 and 2 degrees
    dflt = be.triangulate(pb.x_true, max_iter=0)
    for p in left:
        assert dflt.status[p] in (dflt.FEW_VIEWS, dflt.LOW_ANGLE, dflt.BEHIND) or 1.0 <= tk.angle[p] < 2.0, p
    assert np.all(dflt.status[cmp_] == dflt.OK)


# ---- test 2: the refinement -----------------------------------------------------------------------------------------------

def test_refinement_reaches_the_gauss_newton_fixed_point(be, problem):
    pb, tk, two, cmp_ = problem
    be.set_precision(64)
    be.set_problem(*pb.args)
    lin = be.triangulate(pb.x_true, max_iter=0)
    tri = be.triangulate(pb.x_true)
    assert np.all(tri.status[cmp_] == tri.OK)
    _check_refined(tk, tri, lin.points, cmp_)
    rms = _run_rms(be, tk, tri, cmp_)
    assert np.all(np.abs(tri.rms_err[cmp_] - rms) <= 1e-12 * rms)
    assert tri.n_ok == int((tri.status == 0).sum()) and np.array_equal(tri.ok, tri.status == 0)
    # the restatement takes the same decisions (a one-camera track's DLT lies at its camera centre, where the sign of the
    # depth is rounding: those are test 3's)
    ref = tr.triangulate(pb.x_true, pb.args)
    sure = np.concatenate([cmp_, np.flatnonzero(tk.views < 2)])
    assert np.array_equal(tri.status[sure], ref["status"][sure]) and np.array_equal(tri.views, ref["views"])


# ---- test 3: statuses and pass-through ------------------------------------------------------------------------------------

def test_statuses_and_pass_through(be, problem):
    pb, tk, two, cmp_ = problem
    C, P, ci, pi, uv, K = pb.args
    x = pb.x_true
    pts = x[6 * C:].reshape(P, 3)
    be.set_precision(64)
    be.set_problem(*pb.args)
    one_cam = np.array([p for p in two if len(set(tk.ci[tk.runs[p]])) == 1])
    assert len(one_cam) >= 3
    # one-camera tracks: widest angle 0 (a x a leaves a rounding residue under fused multiply-adds: 1e-9 degrees is the
    # angle bound of the statistics tests).  Without the depth test LOW_ANGLE; with it the verdict before (BEHIND) may
    # win, since their DLT lands next to the camera centre
    tri = be.triangulate(x, min_depth=-np.inf)
    assert np.all(tri.status[one_cam] == tri.LOW_ANGLE) and np.all(tri.angle_deg[one_cam] <= 1e-9)
    assert np.all(np.isin(be.triangulate(x).status[one_cam], (tri.LOW_ANGLE, tri.BEHIND)))
    assert np.array_equal(tri.points[one_cam], pts[one_cam])
    # one used observation, forced through obs_use (caller's order)
    p = int(cmp_[np.argmax(tk.views[cmp_] >= 3)])
    use = np.ones(len(ci), dtype=bool)
    use[tk.runs[p][1:]] = False
    t1 = be.triangulate(x, obs_use=use)
    assert t1.status[p] == t1.FEW_VIEWS and t1.views[p] == 1 and t1.iters[p] == 0 and np.isnan(t1.rms_err[p])
    assert np.array_equal(t1.points[p], pts[p])
    others = np.setdiff1d(np.arange(P), [p])
    full = be.triangulate(x)
    assert np.array_equal(t1.status[others], full.status[others]) and t1.points[others].tobytes() == full.points[others].tobytes()
    # a camera moved in x to the far side of a two-view track, same orientation: the track lies behind it
    q = int(next(p for p in cmp_ if tk.views[p] == 2 and tk.angle[p] >= 5.0))
    cb = int(tk.ci[tk.runs[q][1]])
    xb = x.copy()
    xb[6 * cb + 3:6 * cb + 6] = 2.0 * pts[q] - x[6 * cb + 3:6 * cb + 6]
    sel = np.zeros(P, dtype=bool)
    sel[q] = True
    tb = be.triangulate(xb, select=sel)
    assert tb.status[q] == tb.BEHIND and np.array_equal(tb.points[q], pts[q]) and tb.angle_deg[q] > 1.0
    # unselected points: -1, and their rows are bitwise those of x
    rest = ~sel
    assert np.all(tb.status[rest] == tb.NOT_SELECTED) and np.all(tb.views[rest] == 0) and np.all(tb.iters[rest] == 0)
    assert tb.points[rest].tobytes() == pts[rest].tobytes() and tb.n_ok == 0
    assert full.n_ok == int((full.status == 0).sum()) and 0 < full.n_ok < P


def test_high_error_and_masking_the_outlier(be, problem):
    pb, tk, two, cmp_ = problem
    C, P, ci, pi, uv, K = pb.args
    p = int(cmp_[np.argmax(tk.views[cmp_] >= 5)])
    bad = int(tk.runs[p][2])
    uv2 = np.array(uv, dtype=np.float64)
    uv2[bad] += np.array([160.0, -120.0])                            # 200 px
    use = np.ones(len(ci), dtype=bool)
    use[bad] = False
    be.set_precision(64)
    be.set_problem(C, P, ci, pi, np.asarray(uv, dtype=np.float64), K)
    clean = be.triangulate(pb.x_true, obs_use=use, max_error_px=4.0)
    be.set_problem(C, P, ci, pi, uv2, K)
    hit = be.triangulate(pb.x_true, max_error_px=4.0)
    assert hit.status[p] == hit.HIGH_ERROR and np.array_equal(hit.points[p], pb.x_true[6 * C + 3 * p:6 * C + 3 * p + 3])
    assert hit.rms_err[p] > 4.0
    masked = be.triangulate(pb.x_true, obs_use=use, max_error_px=4.0)
    assert masked.status[p] == masked.OK and masked.views[p] == tk.views[p] - 1
    X, X0 = masked.points[p], clean.points[p]
    assert np.sqrt(((X - X0) ** 2).sum()) <= 100 * XTOL * (np.sqrt(X0 @ X0) + XTOL)
    others = np.setdiff1d(np.arange(P), [p])
    assert np.array_equal(hit.status[others], masked.status[others])


def test_errors(be, problem):
    import sfmba
    pb, tk, two, cmp_ = problem
    empty = sfmba.Backend(0)
    try:
        with pytest.raises(ValueError):
            empty.triangulate(np.zeros(0))
    finally:
        empty.close()
    be.set_precision(64)
    be.set_problem(*pb.args)
    for kw in (dict(xtol=np.nan), dict(min_angle_deg=np.nan), dict(min_depth=np.nan), dict(max_error_px=np.nan)):
        with pytest.raises(ValueError):
            be.triangulate(pb.x_true, **kw)
    with pytest.raises(TypeError):
        be.triangulate(pb.x_true, max_iterations=3)
    with pytest.raises(ValueError):
        be.triangulate(pb.x_true, select=np.ones(tk.P + 1, dtype=bool))
    with pytest.raises(ValueError):
        be.triangulate(pb.x_true, obs_use=np.ones(len(tk.ci) - 1, dtype=bool))
    # the args-tuple wrapper is the same call
    a = sfmba.triangulate_tracks(pb.x_true, pb.args, backend=be, max_iter=3)
    b = be.triangulate(pb.x_true, max_iter=3)
    assert a.points.tobytes() == b.points.tobytes() and np.array_equal(a.status, b.status) and a.n_ok == b.n_ok
    assert be.time_kernel(pb.x_true, 15, 2) > 0.0


# ---- test 4: the run-length switch ------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ring():
    """40 cameras on a ring; tracks of exactly 2, L-1, L, L+1 and 40 views (L = kStatsLongTrack) spread among 700
    three- and four-view tracks: lane- and wave-handled runs in the same waves, more than one workgroup."""
    L = kernel_constant("kStatsLongTrack")
    assert L == 32 and kernel_constant("kTriThreads") < 705
    special = {5: 2, 70: L - 1, 71: L, 300: L + 1, 640: 40}
    x, args = consumer_inputs.ring_tracks(40, 705, special, cam_seed=9, seed=17)
    return x, args, special


def test_lane_and_wave_handled_runs(be, ring):
    x, args, special = ring
    C, P, ci, pi, uv, K = args
    tk = Tracks(x, args)
    sp = np.array(sorted(special))
    assert np.array_equal(tk.views[sp], [special[p] for p in sp]) and tk.angle[sp].min() >= 2.0
    which = np.concatenate([sp, np.arange(0, P, 7)])
    which = which[tk.angle[which] >= 2.0]
    be.set_precision(64)
    be.set_problem(*args)
    lin = be.triangulate(x, max_iter=0, min_angle_deg=2.0)
    assert np.all(lin.status[which] == lin.OK)
    # the restatement's own distance on this geometry is within the recorded one's bound too
    ref_lin = tr.triangulate(x, args, select=np.isin(np.arange(P), sp), max_iter=0)["linear"]
    _check_linear(tk, ref_lin, sp, bound=LIN_REL / BOUNDS["factor"] * 10)
    _check_linear(tk, lin.points, which)
    tri = be.triangulate(x)
    assert np.all(tri.status[which] == tri.OK)
    _check_refined(tk, tri, lin.points, which)
    rms = _run_rms(be, tk, tri, which)
    assert np.all(np.abs(tri.rms_err[which] - rms) <= 1e-12 * rms)
    assert np.abs(tri.angle_deg[which] - np.array([tr.widest_angle_deg(tri.points[p], tk.cams[tk.ci[tk.runs[p]], 3:])
                                                   for p in which])).max() <= 1e-9
    # a second call returns the same bits
    again = be.triangulate(x)
    for name in ("points", "status", "views", "iters", "rms_err", "angle_deg"):
        assert getattr(again, name).tobytes() == getattr(tri, name).tobytes(), name
    # obs_use, in the caller's order: observations taken out of the wave-handled runs and of a lane-handled one
    use = np.ones(len(ci), dtype=bool)
    for p, drop in ((71, (0, 31)), (300, (1, 2, 32)), (640, tuple(range(3, 40, 4))), (70, (30,)), (5, (0,))):
        use[tk.runs[p][list(drop)]] = False
    tku = Tracks(x, args, obs_use=use)
    mu = be.triangulate(x, obs_use=use)
    assert np.array_equal(mu.views, tku.views) and mu.status[5] == mu.FEW_VIEWS
    chk = np.array([70, 71, 300, 640])
    assert np.all(mu.status[chk] == mu.OK)
    lin_u = be.triangulate(x, obs_use=use, max_iter=0)
    _check_linear(tku, lin_u.points, chk)
    _check_refined(tku, mu, lin_u.points, chk)
    # the same problem handed over in a non-point-major order (first observation of every point, then the second, ...:
    # the stored order inside a run is the caller's, so the sums run in the same order): same bits, masks permuted alike
    perm = consumer_inputs.point_interleaved_order(pi)
    assert np.any(np.diff(pi[perm]) < 0)
    be.set_problem(C, P, ci[perm], pi[perm], uv[perm], K)
    sh, shu = be.triangulate(x), be.triangulate(x, obs_use=use[perm])
    for name in ("points", "status", "views", "iters", "rms_err", "angle_deg"):
        assert getattr(sh, name).tobytes() == getattr(tri, name).tobytes(), name
        assert getattr(shu, name).tobytes() == getattr(mu, name).tobytes(), name


def _result_angles(tk, tri, which):
    return np.array([tr.widest_angle_deg(tri.points[p], tk.cams[tk.ci[tk.runs[p]], 3:]) for p in which])


def test_runs_longer_than_a_wave(be):
    """Tracks of 63, 64, 65, 128 and 130 views: the wave form with one, two and three blocks of 64 observations, full and
    partial -- the linear and refined checks of test_lane_and_wave_handled_runs, then again with observations taken out
    of every block of the runs that have more than one."""
    x, args = consumer_inputs.long_run_problem()
    C, P, ci, pi, uv, K = args
    special = consumer_inputs.LONG_RUNS
    tk = Tracks(x, args)
    sp = np.array(sorted(special))
    assert np.array_equal(tk.views[sp], [special[p] for p in sp]) and tk.angle[sp].min() >= 2.0
    be.set_precision(64)
    be.set_problem(*args)
    lin = be.triangulate(x, max_iter=0, min_angle_deg=2.0)
    assert np.all(lin.status[sp] == lin.OK)
    _check_linear(tk, lin.points, sp)
    tri = be.triangulate(x)
    assert np.all(tri.status[sp] == tri.OK)
    _check_refined(tk, tri, lin.points, sp)
    rms = _run_rms(be, tk, tri, sp)
    assert np.all(np.abs(tri.rms_err[sp] - rms) <= 1e-12 * rms)
    assert np.abs(tri.angle_deg[sp] - _result_angles(tk, tri, sp)).max() <= 1e-9
    # obs_use: observations out of both blocks of the 65-view run and out of all of the 128- and the 130-view run's
    use = np.ones(len(ci), dtype=bool)
    for p, drop in ((90, (0, 7, 64)), (130, (3, 63, 64, 70, 127)), (204, (5, 40, 64, 100, 128, 129))):
        assert special[p] > max(drop)
        use[tk.runs[p][list(drop)]] = False
    tku = Tracks(x, args, obs_use=use)
    mu = be.triangulate(x, obs_use=use)
    chk = np.array([90, 130, 204])
    assert np.array_equal(mu.views, tku.views) and np.all(mu.status[chk] == mu.OK)
    lin_u = be.triangulate(x, obs_use=use, max_iter=0)
    _check_linear(tku, lin_u.points, chk)
    _check_refined(tku, mu, lin_u.points, chk)
    assert np.abs(mu.angle_deg[chk] - _result_angles(tku, mu, chk)).max() <= 1e-9


def test_camera_table_too_large_for_the_lds(be):
    """More cameras than the LDS holds a table of: rows read through L2.  A selection of the points, against the SVD."""
    import sfmba
    pb = sfmba.make_problem(1200, 800, 6000, seed=6)
    assert 1200 * kernel_constant("kCamRow") * 8 > 160 * 1024
    sel = np.zeros(800, dtype=bool)
    sel[::5] = True
    tk = Tracks(pb.x_true, pb.args)
    which = np.flatnonzero(sel & (tk.views >= 2) & (tk.angle >= 2.0))
    assert len(which) >= 100
    be.set_precision(64)
    be.set_problem(*pb.args)
    assert be.form("lds_tab") == 0
    lin = be.triangulate(pb.x_true, select=sel, max_iter=0)
    tri = be.triangulate(pb.x_true, select=sel)
    assert np.all(lin.status[which] == lin.OK) and np.all(tri.status[~sel] == tri.NOT_SELECTED)
    _check_linear(tk, lin.points, which)
    _check_refined(tk, tri, lin.points, which)


# ---- test 5: storage and isolation ------------------------------------------------------------------------------------------

def test_fp32_storage_reads_the_rounded_pixels(be, problem):
    pb, tk, two, cmp_ = problem
    C, P, ci, pi, uv, K = pb.args
    uvf = np.asarray(uv, dtype=np.float64) + np.random.default_rng(4).uniform(0.0, 1.0, (len(ci), 2))
    rounded = uvf.astype(np.float32).astype(np.float64)
    assert np.abs(rounded - uvf).max() > 1e-5
    tkr, tkf = Tracks(pb.x_true, (C, P, ci, pi, rounded, K)), Tracks(pb.x_true, (C, P, ci, pi, uvf, K))
    which = np.flatnonzero((tkr.views >= 2) & (tkr.angle >= 2.0))
    try:
        be.set_precision(32)
        be.set_problem(C, P, ci, pi, uvf, K)
        lin, tri = be.triangulate(pb.x_true, max_iter=0), be.triangulate(pb.x_true)
    finally:
        be.set_precision(64)
    assert np.all(lin.status[which] == lin.OK)
    _check_linear(tkr, lin.points, which)
    # ... and not the unrounded ones: those give points further away than the bound on some track
    far = max(np.abs(lin.points[p] - tkf.svd[p]).max() / max(1.0, np.abs(tkf.svd[p]).max()) for p in which)
    assert far > 10 * LIN_REL
    _check_refined(tkr, tri, lin.points, which)
    ref = tr.triangulate(pb.x_true, (C, P, ci, pi, rounded, K))
    assert np.array_equal(tri.status[which], ref["status"][which]) and np.all(tri.status[which] == tri.OK)
    d = np.sqrt(((tri.points[which] - ref["points"][which]) ** 2).sum(axis=1))
    # both within one (bounded) Gauss-Newton step of the same minimiser
    assert np.all(d <= 200 * XTOL * (np.sqrt((ref["points"][which] ** 2).sum(axis=1)) + XTOL))


def test_triangulation_does_not_disturb_a_solve():
    import sfmba
    pb = sfmba.make_problem(8, 120, 900, seed=21)
    use = np.arange(pb.n_obs) % 3 != 0

    def solve(b, before=False, between=False):
        b.set_precision(64)
        b.set_problem(*pb.args)
        if before:
            b.triangulate(pb.x_true, obs_use=use, max_error_px=3.0)
        opt = b.default_options()
        opt.ftol = 1e-10
        xs, res, _, _ = b.solve(pb.x0, opt, want_fun=False, want_grad=False)     # fun, grad stay on the device
        if between:
            kept = b.fetch_fun_grad()
            b.triangulate(pb.x0, select=np.arange(120) % 2 == 0)               # at ANOTHER x than the solve's result
            after = b.fetch_fun_grad()
            assert kept[0].tobytes() == after[0].tobytes() and kept[1].tobytes() == after[1].tobytes()
        fun, grad = b.fetch_fun_grad()
        return xs, res.cost, int(res.nfev), fun, grad

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
        assert got[3].tobytes() == want[3].tobytes() and got[4].tobytes() == want[4].tobytes()


# ---- test 6: refine_reconstruction(retriangulate=True) ------------------------------------------------------------------------

def test_refine_reconstruction_retriangulates_wrecked_points(be):
    """8 cameras, 200 points, 1600 observations with clean pixels; x0 is the truth except for 10 points (each seen at
    least four times under at least 4 degrees) moved 2 units away.  Every round solves for two function evaluations.
    Seed, distance and threshold were fixed on the CPU, with the oracle's solver and the numpy restatement: after the
    first solve every wrecked point has at most one observation under 6 px (the second smallest error of any of them
    is 16.0 px) while no other observation is above 5.2 px, and re-triangulated with the cameras of that solve their
    largest error is 2.3 px; the one other point the round drops opens 1.0 degrees and stays LOW_ANGLE."""
    import sfmba
    pb = sfmba.make_problem(8, 200, 1600, seed=11, x0_noise=0.0)
    C, P, ci, pi, uv, K = pb.args
    tk = Tracks(pb.x_true, pb.args)
    rng = np.random.default_rng(7)
    wreck = np.sort(rng.choice(np.flatnonzero((tk.angle >= 4.0) & (tk.views >= 4)), 10, replace=False))
    off = rng.normal(size=(10, 3))
    off *= 2.0 / np.sqrt((off * off).sum(axis=1))[:, None]
    x0 = pb.x0.copy()
    x0[6 * C:].reshape(P, 3)[wreck] += off
    kw = dict(rounds=2, max_error_px=6.0, min_depth=0.0, min_angle_deg=2.0, min_views=2, ftol=1e-10, max_nfev=2, backend=be)
    result, (x2, args2), (oi, pti), rounds = sfmba.refine_reconstruction(x0, pb.args, retriangulate=True, **kw)
    assert rounds[0]["n_points_retriangulated"] == 10
    assert np.all(np.isin(wreck, pti))
    # their final error, over every observation they still have, is under the threshold
    r = tr.orc.compute_residuals(x2, *args2).reshape(-1, 2)
    mine = np.isin(pti[args2[3]], wreck)
    assert mine.sum() >= 20 and np.sqrt((r[mine] ** 2).sum(axis=1)).max() < 6.0
    assert all("n_points_retriangulated" in s for s in rounds)
    # without the flag the same points are dropped in the first round
    _, _, (_, pti0), rounds0 = sfmba.refine_reconstruction(x0, pb.args, **kw)
    assert not np.isin(wreck, pti0).any() and "n_points_retriangulated" not in rounds0[0]
