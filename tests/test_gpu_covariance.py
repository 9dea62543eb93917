"""sfmba_covariance on the GPU against the two-route CPU reference (tests/covariance_ref.py).  The covariance blocks are held
to factor x the recorded spread of the reference's routes (tests/golden/covariance_bounds.json, written on the CPU by
tools/gen_covariance_golden.py), sigma2 and cost to N 2^-52 relative: what reordering a sum of N non-negative terms can cost.
The reference the blocks are compared with is route B; every case's reference is computed once and shared."""
import numpy as np
import pytest

import covariance_ref as ref

pytestmark = pytest.mark.gpu

MARGINAL = ("c3", "c3_fixed0", "c3_fixed01", "c11", "c11_dup", "c21", "grid21", "grid21_multi")
_refs = {}


@pytest.fixture(scope="module")
def be():
    import sfmba
    b = sfmba.Backend(0)
    yield b
    b.close()


@pytest.fixture(scope="module")
def bounds():
    return ref.load_bounds()


def reference(name):
    if name not in _refs:
        c = ref.case(name)
        _refs[name] = ref.covariance(c["x"], c["args"], fixed=c["fixed"], hold=c["hold"], gauge=c["gauge"], kind=c["kind"])
    return _refs[name]


def run(be, name, **kw):
    c = ref.case(name)
    be.set_precision(64)
    be.set_fixed_cameras(c["fixed"])
    be.set_problem(*c["args"])
    kw.setdefault("kind", "conditional" if c["kind"] else "marginal")
    kw.setdefault("gauge", "auto" if c["gauge"] else "none")
    kw.setdefault("want_full", True)
    return be.covariance(c["x"], **kw)


def check_against_reference(name, got, want, bounds):
    b = bounds["cases"][name]
    f = bounds["factor"]
    c = ref.case(name)
    N = len(c["args"][2])
    assert got.status == 0 and got.ok and want["status"] == 0
    assert got.gauge == tuple(want["gauge"]) == tuple(b["gauge"])
    assert np.array_equal(got.held, want["held"])
    assert (got.n_free, got.n_held, got.dof) == (want["n_free"], want["n_held"], want["dof"]) and got.dof == b["dof"]
    assert np.array_equal(got.pt_status, want["pt_status"])
    e_s2, e_cost = abs(got.sigma2 - want["sigma2"]) / want["sigma2"], abs(got.cost - want["cost"]) / want["cost"]
    e_full, e_cam = ref.block_error(got.cam_full, want["cam_full"]), ref.block_error(got.cam_cov, want["cam_cov"])
    ok = want["pt_status"] == 0
    e_pt = ref.block_error(got.pt_cov[ok], want["pt_cov"][ok])
    print(f"{name}: sigma2 {e_s2:.2e} cost {e_cost:.2e} (bound {N * 2.0 ** -52:.2e}); cam_full {e_full:.2e} cam_cov {e_cam:.2e} "
          f"(bound {f * b['spread_cam']:.2e}); pt_cov {e_pt:.2e} (bound {f * b['spread_pt']:.2e}); "
          f"min pivot {got.min_pivot_rel:.3e} (reference {want['min_pivot_rel']:.3e})")
    assert e_s2 <= N * 2.0 ** -52 and e_cost <= N * 2.0 ** -52
    assert e_full <= f * b["spread_cam"] and e_cam <= f * b["spread_cam_cov"]
    assert e_pt <= f * b["spread_pt"]
    assert np.isnan(got.pt_cov[~ok]).all() and np.isnan(got.pt_sigma[~ok]).all()


def check_structure(got):
    """cam_cov is the diagonal block of cam_full, blocks are symmetric -- bitwise -- and the sigmas are the square roots of
    the blocks' largest eigenvalues: Jacobi and LAPACK are both backward stable, |d lambda| <= c n eps |A| with c n a few
    tens, so 1e-13 relative to lambda_max."""
    Cn = got.cam_cov.shape[0]
    for c in range(Cn):
        assert np.array_equal(got.cam_cov[c], got.cam_full[6 * c:6 * c + 6, 6 * c:6 * c + 6], equal_nan=True)
    assert np.array_equal(got.cam_full, got.cam_full.T, equal_nan=True)
    assert np.array_equal(got.pt_cov, got.pt_cov.transpose(0, 2, 1), equal_nan=True)
    ok = got.pt_status == 0
    lam = np.linalg.eigvalsh(got.pt_cov[ok])[:, -1]
    assert (np.abs(got.pt_sigma[ok] ** 2 - lam) <= 1e-13 * lam).all()
    for k, sl in enumerate((slice(0, 3), slice(3, 6))):
        lam = np.linalg.eigvalsh(got.cam_cov[:, sl, sl])[:, -1]
        assert (np.abs(got.cam_sigma[:, k] ** 2 - lam) <= 1e-13 * np.maximum(lam, 1e-300)).all()


@pytest.mark.parametrize("name", MARGINAL)
def test_marginal_matches_reference(be, bounds, name):
    """n = 18 with the default gauge (0, 1, axis 0), with camera 0 and cameras 0, 1 held by the problem (two held: no gauge
    is added), the three dropped points reporting pt_status = 3; SceauxCastle scale as it is and with one observation
    duplicated (a camera sees a point twice); n = 126, the LDS limit, cam_full entry by entry; the full grid, every track
    21 views, the longest Z_a loop; the grid with cameras that see a point twice and four times: runs of 32, 42 and 84
    observations, which the wave takes (the switch-over is 32; 84 is more than one block of 64)."""
    got = run(be, name)
    check_against_reference(name, got, reference(name), bounds)
    check_structure(got)
    if name == "c3":
        assert got.gauge == (0, 1, 0) and list(np.nonzero(got.pt_status == 3)[0]) == [2, 4, 16]
    if name == "c3_fixed01":
        assert got.gauge == (-1, -1, -1) and got.n_held == 12


def test_undetermined_points_end_the_call(be):
    """Without dropping, the three single-view points of the 3-camera problem have a singular V_p."""
    got = run(be, "c3_undropped")
    want = reference("c3_undropped")
    assert got.status == 2 and want["status"] == 2 and not got.ok
    assert got.n_bad_points == 3 and got.bad_point == 2
    assert list(np.nonzero(got.pt_status == 1)[0]) == [2, 4, 16] and np.array_equal(got.pt_status, want["pt_status"])
    for a in (got.cam_cov, got.cam_full, got.cam_sigma, got.pt_cov, got.pt_sigma):
        assert np.isnan(a).all()
    assert np.array_equal(got.held, want["held"]) and got.gauge == (0, 1, 0)


def test_no_gauge_is_rank_deficient(be):
    """gauge = 0 and nothing held: S has seven null directions.  The first 59 pivots are sound (66 - 7), so the GPU's failing
    index is >= 59; the reference's own Cholesky fails at 59.  Which of the last seven pivots first falls below
    rank_tol S_kk is decided by rounding, so only the fact of the failure is compared."""
    got = run(be, "c11_nogauge")
    want = reference("c11_nogauge")
    assert want["status"] == 1 and want["bad_param"] == 59
    assert got.status == 1 and got.bad_param >= 59 and got.bad_param < 66
    assert got.n_held == 0 and got.gauge == (-1, -1, -1)
    for a in (got.cam_cov, got.cam_full, got.cam_sigma, got.pt_cov, got.pt_sigma):
        assert np.isnan(a).all()
    assert (got.pt_status == 0).all()


def test_hold_list_equals_default_gauge(be):
    """Camera 0's six parameters plus one coordinate of another camera, given explicitly, is the default gauge bit for bit."""
    auto = run(be, "c11")
    g0, g1, axis = auto.gauge
    assert g0 == 0
    idx = [6 * g0 + k for k in range(6)] + [6 * g1 + 3 + axis]
    pairs = [(g0, k) for k in range(6)] + [(g1, 3 + axis)]
    for hold in (idx, pairs):
        got = run(be, "c11", hold=hold)
        assert got.gauge == (-1, -1, -1) and np.array_equal(got.held, auto.held)
        for name in ("cam_cov", "cam_full", "cam_sigma", "pt_cov", "pt_sigma"):
            assert np.array_equal(getattr(got, name), getattr(auto, name)), name
        assert got.sigma2 == auto.sigma2 and got.dof == auto.dof
    # a hold list switches the default gauge off even when it does not fix the gauge: one coordinate leaves six directions
    assert run(be, "c11", hold=[3]).status == 1
    with pytest.raises(ValueError, match="repeated"):
        run(be, "c11", hold=[0, 1, 0])
    for q in (-1, 66):
        with pytest.raises(ValueError, match="out of range"):
            run(be, "c11", hold=[q])


def test_conditional_above_the_dense_limit(be, bounds):
    """40 cameras / 300 points / 2000 observations: kind = 1 against sigma^2 U^-1 and sigma^2 V^-1; kind = 0 is refused and
    the message names the limit."""
    got = run(be, "cond40")
    check_against_reference("cond40", got, reference("cond40"), bounds)
    check_structure(got)
    off = got.cam_full.copy()
    for c in range(40):
        off[6 * c:6 * c + 6, 6 * c:6 * c + 6] = 0.0
    assert not off.any()
    with pytest.raises(ValueError, match="128"):
        run(be, "cond40", kind="marginal")
    assert run(be, "cond40", want_points=False, want_full=False).pt_cov is None      # the handle still works


def test_lds_form_of_the_point_sweep_gives_the_same_bits(be):
    """The point sweep that reads Sigma_cc from L2 ("cov_lds" = 0) adds the same terms in the same order as the form that
    stages it in LDS (the default): lane-handled runs (c21) and wave-handled ones (grid21_multi)."""
    for name in ("c21", "grid21_multi"):
        a = run(be, name)
        be.debug_option("cov_lds", 0)
        try:
            b = run(be, name)
        finally:
            be.debug_option("cov_lds", -1)
        assert np.array_equal(a.pt_cov, b.pt_cov, equal_nan=True) and np.array_equal(a.pt_sigma, b.pt_sigma, equal_nan=True)


def test_properties(be, bounds):
    """Marginal minus conditional point blocks have no eigenvalue below -bound lambda_max; sigma2 = sum r^2 / dof with the
    reference's dof; an explicit sigma2 that is a power of two scales every block exactly linearly."""
    c = ref.case("c11")
    b = bounds["cases"]["c11"]
    marg = run(be, "c11")
    cond = run(be, "c11", kind="conditional")
    diff = marg.pt_cov - cond.pt_cov
    ev = np.linalg.eigvalsh(0.5 * (diff + diff.transpose(0, 2, 1)))
    lam = np.linalg.eigvalsh(marg.pt_cov)[:, -1]
    worst = (ev[:, 0] / lam).min()
    print(f"smallest eigenvalue of marginal - conditional over lambda_max: {worst:.3e} (bound {-bounds['factor'] * b['spread_pt']:.3e})")
    assert worst >= -bounds["factor"] * b["spread_pt"]
    assert (np.linalg.eigvalsh(marg.cam_cov - cond.cam_cov)[:, 0] >= -bounds["factor"] * b["spread_cam"] *
            np.linalg.eigvalsh(marg.cam_cov)[:, -1]).all()
    r = ref.orc.jacobian_blocks(c["x"], *c["args"])[0]
    want = float((r ** 2).sum()) / reference("c11")["dof"]
    assert abs(marg.sigma2 - want) <= len(r) * 2.0 ** -52 * want
    for kind in ("marginal", "conditional"):
        one, four = run(be, "c11", kind=kind, sigma2=1.0), run(be, "c11", kind=kind, sigma2=4.0)
        assert one.sigma2 == 1.0 and four.sigma2 == 4.0
        for name in ("cam_cov", "cam_full", "pt_cov"):
            assert np.array_equal(4.0 * getattr(one, name), getattr(four, name)), (kind, name)
        for name in ("cam_sigma", "pt_sigma"):
            assert np.allclose(2.0 * getattr(one, name), getattr(four, name), rtol=1e-13, atol=0), (kind, name)


def test_handle_state(be):
    """Two calls give the same bits; fun and grad of a solve left on the device are the same bits after a covariance call;
    a solve after a covariance call equals one on a fresh handle: x, nfev and the PCG record."""
    import sfmba
    a, b = run(be, "c11"), run(be, "c11")
    for name in ("cam_cov", "cam_full", "cam_sigma", "pt_cov", "pt_sigma", "pt_status", "held"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    assert (a.sigma2, a.cost, a.min_pivot_rel) == (b.sigma2, b.cost, b.min_pivot_rel)
    pb = sfmba.make_problem(11, 200, 1600, seed=2)

    def solve(h, cov_before=False, cov_between=False):
        h.set_precision(64)
        h.set_fixed_cameras(())
        h.set_problem(*pb.args)
        if cov_before:
            h.covariance(pb.x_true)
        opt = h.default_options()
        opt.ftol = 1e-10
        xs, res, _, _ = h.solve(pb.x0, opt, want_fun=False, want_grad=False)      # fun, grad stay on the device
        if cov_between:
            assert h.covariance(xs, want_full=True).ok
        fun, grad = h.fetch_fun_grad()
        return xs, res.cost, int(res.nfev), h.pcg_history(), fun, grad

    fresh = sfmba.Backend(0)
    try:
        want = solve(fresh)
    finally:
        fresh.close()
    for kw in (dict(cov_between=True), dict(cov_before=True)):
        got = solve(be, **kw)
        assert np.array_equal(got[0], want[0]) and got[1:4] == want[1:4], kw
        assert np.array_equal(got[4], want[4]) and np.array_equal(got[5], want[5]), kw
    # the same through the public calls: least_squares -> covariance(res.x) -> res.fun / res.grad
    res0 = sfmba.least_squares(sfmba.compute_residuals, pb.x0, x_scale="jac", ftol=1e-10, method="trf", args=pb.args)
    fun0, grad0 = np.array(res0.fun), np.array(res0.grad)
    res1 = sfmba.least_squares(sfmba.compute_residuals, pb.x0, x_scale="jac", ftol=1e-10, method="trf", args=pb.args)
    cov = sfmba.covariance(res1.x, *pb.args)
    assert cov.ok and "Covariance(status='ok'" in repr(cov)
    assert np.array_equal(res1.x, res0.x) and np.array_equal(res1.fun, fun0) and np.array_equal(res1.grad, grad0)


def test_error_returns(be):
    import sfmba
    c = ref.case("c3")
    empty = sfmba.Backend(0)
    try:
        with pytest.raises(ValueError):
            empty.covariance(np.zeros(0))
    finally:
        empty.close()
    for kw in (dict(rank_tol=np.nan), dict(point_tol=np.nan), dict(sigma2=np.nan), dict(rank_tol=-1.0), dict(point_tol=-1.0),
               dict(sigma2=-2.0)):
        with pytest.raises(ValueError):
            run(be, "c3", **kw)
    with pytest.raises(TypeError):
        run(be, "c3", tolerance=1.0)
    h = sfmba.Backend(0)
    try:
        h.set_precision(32)
        h.set_problem(*c["args"])
        with pytest.raises(ValueError, match="fp64"):
            h.covariance(c["x"])
        h.set_precision(64)
        h.set_problem(*c["args"])
        assert h.covariance(c["x"]).ok
        assert h.time_kernel(c["x"], 18, 2) > 0.0
    finally:
        h.close()


def test_sharded_world_of_one_is_refused():
    """A handle with a transport attached (the callback transport over a world of one, as tests/test_gpu_step_products.py
    sets it up; importing torch for the arena is what this test's time goes to) holds a shard as far as the library knows."""
    import sfmba
    import torch
    c = ref.case("c3")
    h = sfmba.Backend(0)
    try:
        h.set_problem(*c["args"])
        arena = torch.zeros(h.exchange_doubles(), dtype=torch.float64, device="cuda:0")
        h.set_exchange(arena.data_ptr(), arena.numel(), lambda dev_ptr, count, op: None, len(c["args"][2]))
        with pytest.raises(ValueError, match="shard"):
            h.covariance(c["x"])
        h.set_exchange(0, 0, None, 0)
        assert h.covariance(c["x"]).ok
    finally:
        h.close()
