"""GPU tests of the reprojection statistics (sfmba_reprojection_stats): the three sweeps against numpy on the oracle's
residuals and camera-frame points.  Bounds are stated where used; the arithmetic is fp64 everywhere, pixels are read as
stored (fp64 or fp32)."""
import numpy as np
import pytest

import consumer_inputs
from kernel_source import kernel_constant

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    import sfmba
    b = sfmba.Backend(0)
    yield b
    b.close()


@pytest.fixture(scope="module")
def orc():
    from oracle import ba_oracle
    return ba_oracle


class Ref:
    """numpy expectation at x.  Per-point quantities by a loop over the points (all pairs of rays as one array per point)."""

    def __init__(self, orc, x, args, max_error_px=np.inf, min_depth=-np.inf, min_angle_deg=0.0, min_views=0, angles=True):
        C, P, ci, pi, uv, K = args
        x = np.asarray(x, dtype=np.float64)
        with np.errstate(all="ignore"):
            r = orc.compute_residuals(x, C, P, ci, pi, uv, K).reshape(-1, 2)
            self.err = np.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1])
            cams, pts = x[:6 * C].reshape(C, 6), x[6 * C:].reshape(P, 3)
            self.v = pts[pi] - cams[ci, 3:]                              # the rays X_p - T_c
            self.depth = np.einsum("nj,nj->n", orc.rodrigues(cams[:, :3])[ci][:, 2, :], self.v)
            self.own = (self.err <= max_error_px) & np.isfinite(self.err) & (self.depth > min_depth)
        self.pt_views = np.bincount(pi[self.own], minlength=P).astype(np.int32)
        self.pt_max_err, self.pt_sum_err2 = np.zeros(P), np.zeros(P)
        self.pt_min_depth, self.pt_angle = np.full(P, np.inf), np.zeros(P)
        order = np.argsort(pi, kind="stable")                            # stored order: by point, caller's order inside
        ptr = np.searchsorted(pi[order], np.arange(P + 1))
        for p in range(P):
            idx = order[ptr[p]:ptr[p + 1]]
            if len(idx) == 0:
                continue
            self.pt_min_depth[p] = self.depth[idx].min()
            k = idx[self.own[idx]]
            if len(k) == 0:
                continue
            e = self.err[k]
            self.pt_max_err[p] = e.max()
            s = 0.0
            for q in e:                                                  # stored order
                s += q * q
            self.pt_sum_err2[p] = s
            if angles and len(k) >= 2:
                a = self.v[k]
                cr = np.cross(a[:, None, :], a[None, :, :])
                self.pt_angle[p] = np.degrees(np.arctan2(np.sqrt((cr * cr).sum(axis=2)), a @ a.T)).max()
        self.pt_keep = (self.pt_views >= min_views) & (self.pt_angle >= min_angle_deg)
        self.fin = self.own & self.pt_keep[pi]
        self.cam_views = np.bincount(ci[self.fin], minlength=C).astype(np.int32)
        self.cam_sum_err = np.bincount(ci[self.fin], weights=self.err[self.fin], minlength=C)
        self.cam_max_err = np.zeros(C)
        np.maximum.at(self.cam_max_err, ci[self.fin], self.err[self.fin])
        self.cam_behind = np.bincount(ci[self.depth <= 0.0], minlength=C).astype(np.int32)


def _check_parity(be, orc, x, args, ref, st, residual_rel=1e-14, angles=True):
    """The assertions of the issue's test 1, for statistics `st` taken at `x` and the numpy expectation `ref`."""
    C, P, ci, pi, uv, K = args
    # err against the library's own residual at the same x
    r = be.residuals(x).reshape(-1, 2)
    e_r = np.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1])
    fin_e = np.isfinite(e_r)
    assert np.all(np.abs(st.obs_err[fin_e] - e_r[fin_e]) <= residual_rel * e_r[fin_e])
    # ... against the oracle: the bound test_gpu_parity.py uses for residuals
    fe = np.isfinite(ref.err)
    tol = 1e-11 * max(1.0, float(np.abs(ref.err[fe]).max()), 3000.0)
    assert np.abs(st.obs_err[fe] - ref.err[fe]).max() <= tol
    # depth: relative 1e-12 (of the largest depth, as _rel of test_gpu_parity.py), and per entry of the ray's length,
    # the scale of the three products the depth is the sum of
    fd = np.isfinite(ref.depth)
    assert np.abs(st.obs_depth[fd] - ref.depth[fd]).max() <= 1e-12 * np.abs(ref.depth[fd]).max()
    assert np.all(np.abs(st.obs_depth[fd] - ref.depth[fd]) <= 1e-12 * np.sqrt((ref.v[fd] ** 2).sum(axis=1)))
    # masks, counts: exact
    assert np.array_equal(st.obs_keep, ref.fin)
    assert np.array_equal(st.pt_keep, ref.pt_keep)
    assert np.array_equal(st.pt_views, ref.pt_views)
    assert np.array_equal(st.cam_views, ref.cam_views)
    assert np.array_equal(st.cam_behind, ref.cam_behind)
    assert st.obs_keep.dtype == np.bool_ and st.pt_views.dtype == np.int32 and st.cam_behind.dtype == np.int32
    # max / min: those of the GPU's own per-observation outputs, bit for bit (own test recomputed from them)
    own_gpu = ref.own                                              # (the GPU's too: no decision sits within rounding of a
    gmax, gmin = np.zeros(P), np.full(P, np.inf)                   #  threshold, and obs_keep == ref.fin was asserted)
    np.maximum.at(gmax, pi[own_gpu], st.obs_err[own_gpu])
    np.minimum.at(gmin, pi, st.obs_depth)
    assert np.array_equal(st.pt_max_err, gmax)
    assert np.array_equal(st.pt_min_depth, gmin)
    cmax = np.zeros(C)
    np.maximum.at(cmax, ci[st.obs_keep], st.obs_err[st.obs_keep])
    assert np.array_equal(st.cam_max_err, cmax)
    assert st.max_err == (st.obs_err[st.obs_keep].max() if st.obs_keep.any() else 0.0)
    # sums: relative 1e-13 -- of numpy's sums of the GPU's own per-observation err, which is what the reductions add up.
    # (Against the oracle's err no sum can hold 1e-13: a sub-pixel err agrees with the oracle's to `tol` above, 3e-8 px
    # absolute, a relative 1e-7 of itself.)  Against the oracle the bound is that per-observation bound carried through
    # the sum: n tol for a sum of err, sum 2 err tol for a sum of err^2.
    eg, fin = st.obs_err, st.obs_keep
    g_s2 = np.bincount(pi[own_gpu], weights=eg[own_gpu] ** 2, minlength=P)
    g_cs = np.bincount(ci[fin], weights=eg[fin], minlength=C)
    assert np.all(np.abs(st.pt_sum_err2 - g_s2) <= 1e-13 * g_s2)
    assert np.all(np.abs(st.cam_sum_err - g_cs) <= 1e-13 * g_cs)
    assert abs(st.sum_err - eg[fin].sum()) <= 1e-13 * eg[fin].sum()
    assert abs(st.sum_err2 - (eg[fin] ** 2).sum()) <= 1e-13 * (eg[fin] ** 2).sum()
    slack = 1e-13
    assert np.all(np.abs(st.pt_sum_err2 - ref.pt_sum_err2)
                  <= slack * ref.pt_sum_err2 + np.bincount(pi[own_gpu], weights=2 * tol * ref.err[own_gpu], minlength=P))
    assert np.all(np.abs(st.cam_sum_err - ref.cam_sum_err) <= slack * ref.cam_sum_err + tol * ref.cam_views)
    assert abs(st.sum_err - ref.err[ref.fin].sum()) <= slack * ref.err[ref.fin].sum() + tol * ref.fin.sum()
    assert abs(st.sum_err2 - (ref.err[ref.fin] ** 2).sum()) <= slack * (ref.err[ref.fin] ** 2).sum() + 2 * tol * ref.err[ref.fin].sum()
    # angles: absolute 1e-9 degrees
    if angles:
        assert np.abs(st.pt_max_angle_deg - ref.pt_angle).max() <= 1e-9
    # summary and derived values
    assert st.n_obs == len(ci) and st.n_obs_kept == int(ref.fin.sum()) and st.n_points_kept == int(ref.pt_keep.sum())
    assert st.n_behind == int((ref.depth <= 0.0).sum())
    nk = max(st.n_obs_kept, 1)
    assert st.mean_error_px == st.sum_err / nk and st.rms_error_px == float(np.sqrt(st.sum_err2 / nk))
    assert np.array_equal(st.cam_mean_err, st.cam_sum_err / np.maximum(st.cam_views, 1))


# ---- the small irregular problem of tests 1, 2, 4, 5 ------------------------------------------------------------------

def _irregular_problem(seed=7):
    """~70 cameras, 300 points, 3000 observations (make_problem) plus: point 0 seen by every camera (a run longer than a
    wave), a point seen once, a point never observed, a camera without observations, a duplicated (camera, point) pair,
    camera 5 turned round (negative depths); observations in shuffled order."""
    from sfmba import make_problem
    pb = make_problem(70, 300, 3000, seed=seed)
    rng = np.random.default_rng(seed + 1)
    C, P = 71, 302                                                 # camera 70: no observations; point 301: never observed
    cams = np.vstack([pb.x0[:6 * 70].reshape(70, 6), [[0.01, -0.02, 0.03, 0.1, 0.2, -0.3]]])
    pts = np.vstack([pb.x0[6 * 70:].reshape(300, 3), [[0.3, -0.2, 10.5], [0.0, 0.0, 9.0]]])
    cams[5, :3] = [0.0, np.pi, 0.0]                                # R = diag(-1, 1, -1): looks away from the scene
    ci = np.concatenate([pb.camera_indices, np.arange(70), [12], pb.camera_indices[:1]])
    pi = np.concatenate([pb.point_indices, np.zeros(70, dtype=np.int64), [300], pb.point_indices[:1]])
    uv = np.vstack([pb.points_2d, rng.integers(0, 2800, (70, 2)), [[1500, 1100]], pb.points_2d[:1] + 3]).astype(np.float64)
    uv += rng.uniform(-0.5, 0.5, uv.shape)                         # pixels that fp32 would round
    perm = rng.permutation(len(ci))
    x = np.concatenate([cams.ravel(), pts.ravel()])
    return x, (C, P, ci[perm].astype(np.int64), pi[perm].astype(np.int64), uv[perm], pb.K)


@pytest.fixture(scope="module")
def irregular(orc):
    x, args = _irregular_problem()
    return x, args, Ref(orc, x, args)


def test_parity_small_irregular_problem(be, orc, irregular):
    x, args, ref = irregular
    C, P, ci, pi, uv, K = args
    assert np.bincount(pi, minlength=P)[0] > 64 and np.bincount(pi, minlength=P)[300] == 1       # the problem is as described
    assert np.bincount(pi, minlength=P)[301] == 0 and np.bincount(ci, minlength=C)[70] == 0
    assert np.any(np.diff(pi) < 0)                                                               # not point-major
    assert (ref.depth[ci == 5] < 0).all() and len(np.unique(np.stack([ci, pi]), axis=1)[0]) < len(ci)
    be.set_precision(64)
    be.set_problem(*args)
    st = be.reprojection_stats(x)
    _check_parity(be, orc, x, args, ref, st)
    # defaults: a pure statistics pass
    assert st.obs_keep.all() and st.pt_keep.all() and st.n_obs_kept == st.n_obs
    # the point nobody observes, the camera that observes nothing
    assert st.pt_views[301] == 0 and st.pt_max_err[301] == 0 and st.pt_sum_err2[301] == 0
    assert st.pt_min_depth[301] == np.inf and st.pt_max_angle_deg[301] == 0
    assert st.pt_max_angle_deg[300] == 0 and st.pt_views[300] == 1
    assert st.cam_views[70] == 0 and st.cam_sum_err[70] == 0 and st.cam_max_err[70] == 0 and st.cam_behind[70] == 0
    assert st.cam_behind[5] == np.count_nonzero(ci == 5)
    # the one-call form and the reference's printed figure (divided by N, not N - 1)
    import sfmba
    st2 = sfmba.reprojection_stats(x, args, want=("points",), backend=be)
    assert st2.obs_err is None and st2.cam_views is None and np.array_equal(st2.pt_max_angle_deg, st.pt_max_angle_deg)
    assert sfmba.total_mean_reproj_error(x, args, backend=be) == st.sum_err / st.n_obs


def _widest_gap(values, lo_q, hi_q):
    """Midpoint and width of the widest gap between neighbouring values inside the [lo_q, hi_q] quantile range."""
    v = np.unique(values[np.isfinite(values)])
    v = v[int(lo_q * len(v)):max(int(hi_q * len(v)), int(lo_q * len(v)) + 2)]
    k = int(np.argmax(np.diff(v)))
    return 0.5 * (v[k] + v[k + 1]), float(v[k + 1] - v[k])


def test_threshold_masks(be, orc, irregular):
    x, args, ref0 = irregular
    C, P, ci, pi, uv, K = args
    # every threshold in the middle of the widest gap of the CPU values it cuts: no rounding can flip a decision
    max_err, gap_e = _widest_gap(ref0.err, 0.80, 0.95)
    min_depth, gap_d = _widest_gap(ref0.depth, 0.05, 0.15)
    assert gap_e > 1e-6 and gap_d > 1e-6
    min_views = 3
    ref1 = Ref(orc, x, args, max_err, min_depth, 0.0, min_views)
    min_angle, gap_a = _widest_gap(ref1.pt_angle[ref1.pt_views >= min_views], 0.02, 0.15)
    assert gap_a > 1e-6
    ref = Ref(orc, x, args, max_err, min_depth, min_angle, min_views)
    # some of each kind (on the CPU): observations failing on error, on depth; points failing on views, on angle
    n_err = np.count_nonzero((ref.err > max_err) & (ref.depth > min_depth))
    n_depth = np.count_nonzero((ref.err <= max_err) & (ref.depth <= min_depth))
    n_views = np.count_nonzero(ref.pt_views < min_views)
    n_angle = np.count_nonzero((ref.pt_views >= min_views) & (ref.pt_angle < min_angle))
    assert n_err > 0 and n_depth > 0 and n_views > 0 and n_angle > 0, (n_err, n_depth, n_views, n_angle)
    assert ref.pt_keep.any() and np.count_nonzero(ref.own & ~ref.fin) > 0      # kept observations of dropped points
    be.set_precision(64)
    be.set_problem(*args)
    st = be.reprojection_stats(x, max_error_px=max_err, min_depth=min_depth, min_angle_deg=min_angle, min_views=min_views)
    _check_parity(be, orc, x, args, ref, st)


# ---- test 3: work-unit boundaries -------------------------------------------------------------------------------------

def _boundary_problem():
    x, args = consumer_inputs.boundary_problem()
    return x, args, kernel_constant("kStatsLongTrack")


@pytest.mark.parametrize("bits", [64, 32])
def test_work_unit_boundaries(be, orc, bits):
    x, args, L = _boundary_problem()
    C, P, ci, pi, uv, K = args
    lens = np.bincount(pi, minlength=P)
    assert {L - 1, L, L + 1} <= set(lens.tolist()) and 9000 < len(ci) < 12000
    # fp32 storage: the kernel reads the pixels as stored
    uv_seen = uv.astype(np.float32).astype(np.float64) if bits == 32 else uv
    if bits == 32:
        assert np.any(uv_seen != uv)
    args_seen = (C, P, ci, pi, uv_seen, K)
    thr = dict(max_error_px=1.6, min_depth=0.0, min_angle_deg=0.0, min_views=2)
    ref = Ref(orc, x, args_seen, 1.6, 0.0, 0.0, 2)
    assert np.abs(ref.err - 1.6).min() > 1e-6                        # no decision within rounding of the threshold
    assert 0 < np.count_nonzero(~ref.own) < len(ci) and 0 < np.count_nonzero(~ref.pt_keep) < P
    try:
        be.set_precision(bits)
        be.set_problem(*args)
        st = be.reprojection_stats(x, **thr)
        # (fp32 storage hands residuals back rounded to fp32: each component to 2^-24 relative)
        _check_parity(be, orc, x, args_seen, ref, st, residual_rel=1e-14 if bits == 64 else 2.0 ** -22)
    finally:
        be.set_precision(64)


def test_runs_longer_than_a_wave(be, orc):
    """Runs of 63, 64, 65, 128 and 130 observations: the wave form of the per-point reduction with one, two and three
    blocks, full and partial, a threshold that takes observations out of every block -- against numpy at the bounds of
    test_work_unit_boundaries, and with the observations handed over in another order bit for bit."""
    x, args = consumer_inputs.long_run_problem()
    C, P, ci, pi, uv, K = args
    special = consumer_inputs.LONG_RUNS
    assert all(np.count_nonzero(pi == p) == n for p, n in special.items()) and np.all(np.diff(pi) >= 0)
    thr = dict(max_error_px=1.0, min_depth=0.0, min_angle_deg=0.0, min_views=2)
    ref = Ref(orc, x, args, 1.0, 0.0, 0.0, 2)
    assert np.abs(ref.err - 1.0).min() > 1e-6                        # no decision within rounding of the threshold
    for p, n in special.items():                                     # dropped and kept observations in every block
        own = ref.own[pi == p]                                       # (but for the one or two of a last block)
        for b0 in range(0, n - 2, 64):
            assert 0 < np.count_nonzero(own[b0:b0 + 64]) < len(own[b0:b0 + 64]), (p, b0)
    be.set_precision(64)
    be.set_problem(*args)
    st = be.reprojection_stats(x, **thr)
    _check_parity(be, orc, x, args, ref, st)
    perm = consumer_inputs.point_interleaved_order(pi)
    assert np.any(np.diff(pi[perm]) < 0)
    be.set_problem(C, P, ci[perm], pi[perm], uv[perm], K)
    sh = be.reprojection_stats(x, **thr)
    for name in st._ARRAYS:
        a, b = getattr(st, name), getattr(sh, name)
        assert (a[perm] if name.startswith("obs_") else a).tobytes() == b.tobytes(), name
    for name in st._SUMMARY:
        assert getattr(st, name) == getattr(sh, name), name


def _large_case(which):
    from sfmba import make_problem
    if which == "grid_stride":      # more observations than one pass of the persistent workgroups (256 CUs x 1024 lanes) takes
        return make_problem(300, 60000, 256 * kernel_constant("kSweepThreads") * 2 + 777, seed=5), 40.0
    return make_problem(1200, 800, 6000, seed=6), 40.0      # "many_cameras": the camera table does not fit the LDS


@pytest.mark.parametrize("which", ["grid_stride", "many_cameras"])
def test_other_forms_of_the_observation_sweep(be, orc, which):
    """The forms of the per-observation sweep the small problems do not reach: its software pipeline advancing over
    several batches per lane, and camera rows gathered through the LDS instead of a staged table.  Per-observation
    outputs, counts, sums and the summary against numpy (vectorised: no angles)."""
    pb, thr = _large_case(which)
    x, args = pb.x0, pb.args
    C, P, ci, pi, uv, K = args
    n = len(ci)
    if which == "many_cameras":
        assert C * kernel_constant("kCamRow") * 8 > 160 * 1024
    r = orc.compute_residuals(x, *args).reshape(-1, 2)
    err = np.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1])
    fin = err <= thr
    assert np.abs(err - thr).min() > 1e-6 and 0 < fin.sum() < n
    be.set_precision(64)
    be.set_problem(*args)
    st = be.reprojection_stats(x, max_error_px=thr)
    assert np.abs(st.obs_err - err).max() <= 1e-11 * max(float(err.max()), 3000.0)
    rg = be.residuals(x).reshape(-1, 2)
    eg = np.sqrt(rg[:, 0] * rg[:, 0] + rg[:, 1] * rg[:, 1])
    assert np.all(np.abs(st.obs_err - eg) <= 1e-14 * eg)
    assert np.array_equal(st.obs_keep, fin) and st.pt_keep.all()
    assert np.array_equal(st.pt_views, np.bincount(pi[fin], minlength=P))
    assert np.array_equal(st.cam_views, np.bincount(ci[fin], minlength=C))
    s2 = np.bincount(pi[fin], weights=st.obs_err[fin] ** 2, minlength=P)      # (sums of the GPU's own err: see _check_parity)
    assert np.all(np.abs(st.pt_sum_err2 - s2) <= 1e-13 * s2)
    cs = np.bincount(ci[fin], weights=st.obs_err[fin], minlength=C)
    assert np.all(np.abs(st.cam_sum_err - cs) <= 1e-13 * cs)
    assert st.n_obs_kept == int(fin.sum()) and abs(st.sum_err - st.obs_err[fin].sum()) <= 1e-13 * st.obs_err[fin].sum()
    assert st.max_err == st.obs_err[st.obs_keep].max() and st.n_behind == 0


# ---- test 4: determinism and non-interference -------------------------------------------------------------------------

def _arrays(st):
    return [getattr(st, n) for n in st._ARRAYS] + [np.array([getattr(st, n) for n in st._SUMMARY], dtype=np.float64)]


def test_two_calls_return_identical_bits(be, irregular):
    x, args, _ = irregular
    be.set_precision(64)
    be.set_problem(*args)
    kw = dict(max_error_px=500.0, min_depth=0.0, min_angle_deg=1.0, min_views=2)
    a, b = be.reprojection_stats(x, **kw), be.reprojection_stats(x, **kw)
    for u, v in zip(_arrays(a), _arrays(b)):
        assert u.tobytes() == v.tobytes()


def test_statistics_do_not_disturb_a_solve(be):
    import sfmba
    pb = sfmba.make_problem(8, 120, 900, seed=21)

    def solve(b, stats_before=False, stats_between=False):
        b.set_precision(64)
        b.set_problem(*pb.args)
        if stats_before:
            b.reprojection_stats(pb.x_true, max_error_px=3.0, min_views=2)
        opt = b.default_options()
        opt.ftol = 1e-10
        xs, res, _, _ = b.solve(pb.x0, opt, want_fun=False, want_grad=False)     # fun, grad stay on the device
        if stats_between:
            b.reprojection_stats(pb.x0, max_error_px=3.0, min_views=2)           # at ANOTHER x than the solve's result
        fun, grad = b.fetch_fun_grad()
        return xs, res.cost, int(res.nfev), fun, grad

    fresh = sfmba.Backend(0)
    try:
        want = solve(fresh)
    finally:
        fresh.close()
    for kw in (dict(stats_between=True), dict(stats_before=True)):
        other = sfmba.Backend(0)
        try:
            got = solve(other, **kw)
        finally:
            other.close()
        assert got[0].tobytes() == want[0].tobytes() and got[1] == want[1] and got[2] == want[2], kw
        assert got[3].tobytes() == want[3].tobytes() and got[4].tobytes() == want[4].tobytes(), kw


# ---- test 5: errors -----------------------------------------------------------------------------------------------------

def test_errors(be, irregular):
    import sfmba
    x, args, ref = irregular
    C, P, ci, pi, uv, K = args
    empty = sfmba.Backend(0)
    try:
        with pytest.raises(ValueError):
            empty.reprojection_stats(np.zeros(0))
    finally:
        empty.close()
    be.set_precision(64)
    be.set_problem(*args)
    for kw in (dict(max_error_px=np.nan), dict(min_depth=np.nan), dict(min_angle_deg=np.nan)):
        with pytest.raises(ValueError):
            be.reprojection_stats(x, **kw)
    with pytest.raises(ValueError):
        be.reprojection_stats(x, want=("tracks",))
    # a non-finite x is no error: what it reaches is not kept, the rest is as before
    xb = x.copy()
    xb[6 * 3 + 4] = np.nan                                          # camera 3
    xb[6 * C + 3 * 17 + 1] = np.inf                                 # point 17
    hit = (ci == 3) | (pi == 17)
    st = be.reprojection_stats(xb)
    assert not st.obs_keep[hit].any() and not np.isfinite(st.obs_err[hit]).any()
    assert st.obs_keep[~hit].all() and np.array_equal(st.obs_err[~hit], be.reprojection_stats(x).obs_err[~hit])
    assert st.n_obs_kept == np.count_nonzero(~hit) and np.isfinite(st.sum_err)


# ---- test 6: the trim loop end to end ---------------------------------------------------------------------------------

def test_refine_reconstruction_drops_the_injected_outliers(be):
    """SceauxCastle-scale: 11 cameras, 200 points, 4000 observations with 0.5 px noise, 80 of them (2 %) displaced by
    100-300 px.  Seed and threshold were fixed after the CPU oracle's solve + numpy statistics had been seen to separate
    the two populations at 70 px in every round: after the first solve the injected observations have errors from
    91.6 px up and all others at most 45.6 px; after the second (3920 observations) the largest error is 2.2 px."""
    import sfmba
    pb = sfmba.make_problem(11, 200, 4000, seed=3, pixel_noise=0.5)
    rng = np.random.default_rng(1003)
    N = pb.n_obs
    bad = rng.choice(N, N // 50, replace=False)
    uv = pb.points_2d.copy()
    ang, mag = rng.uniform(0, 2 * np.pi, len(bad)), rng.uniform(100, 300, len(bad))
    uv[bad] += np.trunc(np.stack([mag * np.cos(ang), mag * np.sin(ang)], 1)).astype(np.int64)
    injected = np.zeros(N, dtype=bool)
    injected[bad] = True
    args = (11, 200, pb.camera_indices, pb.point_indices, uv, pb.K)
    result, (x2, args2), (oi, pti), rounds = sfmba.refine_reconstruction(
        pb.x0, args, rounds=3, max_error_px=70.0, min_depth=0.0, min_angle_deg=0.0, min_views=2, ftol=1e-10, backend=be)
    kept = np.zeros(N, dtype=bool)
    kept[oi] = True
    pt_kept = np.zeros(200, dtype=bool)
    pt_kept[pti] = True
    # every dropped observation is an injected one or belongs to a dropped point; every injected one is dropped
    assert np.all(injected[~kept] | ~pt_kept[pb.point_indices[~kept]])
    assert not kept[injected].any()
    # the index maps recover the original rows
    assert np.array_equal(args2[2], pb.camera_indices[oi]) and np.array_equal(args2[4], uv[oi])
    assert np.array_equal(pti[args2[3]], pb.point_indices[oi]) and args2[1] == len(pti) and args2[0] == 11
    assert np.array_equal(x2, result.x) and len(x2) == 66 + 3 * len(pti)
    # first round above 1 px, final RMSE over the kept set below, and the last round drops nothing
    assert len(rounds) == 2
    assert rounds[0]["rmse"] > 1.0 and rounds[0]["n_obs_kept"] < rounds[0]["n_obs"]
    assert rounds[-1]["rms_error_px"] < 1.0 and result.rmse < 1.0
    assert rounds[-1]["n_obs_kept"] == rounds[-1]["n_obs"] == len(oi)
    assert rounds[-1]["n_points_kept"] == rounds[-1]["n_points"] == len(pti)
