"""The host is off a solve's critical path at three places (debug options spec_scale, start_handoff, early_download:
k_update_scale enqueued before the verdict on the trial point, a start without a blocking read-back, the result copied
while the last kernels run).  None of them may change a bit of any result: every case here runs on one handle with the
three options at 0 (the order of launches and copies they replace) and on one with the defaults, and compares x, cost,
optimality, status, nfev, njev, the PCG iteration count, fun and grad with ``np.array_equal``.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OPTIONS = ("spec_scale", "start_handoff", "early_download")


@pytest.fixture
def be():
    """make(off, **debug) -> a fresh Backend, the three options at 0 when `off`; all are closed afterwards."""
    import sfmba
    made = []

    def make(off, **debug):
        b = sfmba.Backend(0)
        made.append(b)
        for name in OPTIONS:
            b.debug_option(name, 0 if off else -1)
        for name, value in debug.items():
            b.debug_option(name, value)
        return b
    yield make
    for b in made:
        b.close()


@pytest.fixture
def dbg(be):
    """pair(**debug) -> (options-off handle, default handle) with the same other debug options."""
    def pair(**debug):
        return be(True, **debug), be(False, **debug)
    return pair


def _solve(b, pb, x0=None, **kw):
    import sfmba
    kw.setdefault("ftol", 1e-10)
    res = sfmba.least_squares(sfmba.compute_residuals, pb.x0 if x0 is None else x0, x_scale="jac", method="trf",
                              args=pb.args, backend=b, **kw)
    fun, grad = np.array(res.fun), np.array(res.grad)        # (downloaded now: the next solve overwrites them)
    return res, fun, grad


def _same(a, b, what):
    (ra, fa, ga), (rb, fb, gb) = a, b
    got = (ra.status, ra.nfev, ra.njev, ra.pcg_iterations), (rb.status, rb.nfev, rb.njev, rb.pcg_iterations)
    print(what, got[1], "cost", rb.cost, "optimality", rb.optimality)
    assert got[0] == got[1], what
    assert ra.cost == rb.cost and ra.optimality == rb.optimality, what
    assert np.array_equal(ra.x, rb.x), what
    assert np.array_equal(fa, fb), what
    assert np.array_equal(ga, gb), what


def _problems():
    import sfmba
    yield "cfg2", sfmba.make_config("cfg2")
    yield "cfg3", sfmba.make_config("cfg3")
    yield "cfg4", sfmba.make_config("cfg4")
    yield "1300 cameras", sfmba.make_problem(1300, 4000, 40000, seed=21)


@pytest.mark.parametrize("bits", [64, 32])
def test_first_and_replayed_solve_at_every_size(dbg, bits):
    """cfg2 (dense reduced camera matrix), cfg3, cfg4 (fused PCG) and more than 1100 cameras (tables in global memory),
    fp64 and fp32 storage: the first solve on a fresh handle and the solve that replays its PCG record."""
    for name, pb in _problems():
        off, on = dbg()
        for k in ("first", "replayed"):
            a = _solve(off, pb, storage_bits=bits)
            b = _solve(on, pb, storage_bits=bits)
            _same(a, b, f"{name} fp{bits} {k}")
            assert np.all(np.isfinite(b[0].x)) and b[0].njev > 1


@pytest.mark.parametrize("dense", [True, False])
def test_rejected_trials_and_solves_that_end_on_one(dbg, dense):
    """Far starts: the speculative k_update_scale of a rejected trial must leave si, g and D^2 g of the accepted point
    alone -- a retry re-applies the step to D^2 g, and a solve that ENDS on a rejected trial returns that g as grad and
    its maximum as optimality.  max_nfev = 5 and 9 (implicit product) / 4 and 11 (dense) end on a rejected trial
    according to the CPU oracle: njev is the one of max_nfev - 1."""
    import sfmba
    debug = {} if dense else {"dense": 0}
    rejected = False
    for seed in (1, 2, 5):
        pb = sfmba.make_problem(6, 80, 500, seed=seed, x0_noise=0.2)
        off, on = dbg(**debug)
        a, b = _solve(off, pb), _solve(on, pb)
        _same(a, b, f"seed {seed} dense {dense}")
        rejected |= b[0].nfev > b[0].njev
    assert rejected
    pb = sfmba.make_problem(6, 80, 500, seed=5, x0_noise=0.2)
    njev = {}
    for max_nfev in range(2, 14):
        off, on = dbg(**debug)
        a, b = _solve(off, pb, max_nfev=max_nfev), _solve(on, pb, max_nfev=max_nfev)
        _same(a, b, f"max_nfev {max_nfev} dense {dense}")
        assert b[0].nfev == max_nfev and b[0].status == 0
        njev[max_nfev] = b[0].njev
    for max_nfev in ((4, 11) if dense else (5, 9)):
        assert njev[max_nfev] == njev[max_nfev - 1], (max_nfev, njev)      # the last trial was not accepted


@pytest.mark.parametrize("dense", [True, False])
def test_non_finite_trial_point(dbg, dense):
    """trf.py:504-506 on the speculative path: K3 and the speculative k_update_scale run on non-finite blocks while the
    host waits; nothing of it may reach the accepted point's vectors."""
    import sfmba
    from sfmba.synthetic import make_plane_crossing_problem
    debug = {} if dense else {"dense": 0}
    for seed, quanta in (((0, 1), (0, 2), (8, 3)) if dense else ((3, 3), (10, 2), (11, 1))):
        pb = make_plane_crossing_problem(seed, quanta)
        S = sfmba.create_sparsity_matrix(pb.n_cameras, pb.n_points, pb.n_obs, pb.camera_indices, pb.point_indices,
                                         fixed_camera_indices=(0,))
        for max_nfev in (12, 2):
            off, on = dbg(**debug)
            a = _solve(off, pb, jac_sparsity=S, xtol=None, max_nfev=max_nfev)
            b = _solve(on, pb, jac_sparsity=S, xtol=None, max_nfev=max_nfev)
            _same(a, b, f"plane crossing {seed, quanta} max_nfev {max_nfev} dense {dense}")
            assert b[0].nfev == max_nfev
            assert np.all(np.isfinite(b[0].x)) and np.all(np.isfinite(b[1])) and np.all(np.isfinite(b[2]))


def test_pcg_miss_cancels_the_speculative_scale_launch(dbg):
    """pcg_guess_bias = -5: every speculative PCG batch falls short, k_tr_step cancels the trial launches -- the
    speculative k_update_scale among them, which would otherwise read blocks K3 never wrote."""
    import sfmba
    for pb in (sfmba.make_config("cfg2"), sfmba.make_problem(6, 80, 500, seed=5, x0_noise=0.2)):
        off, on = dbg(dense=0, pcg_guess_bias=-5)
        for k in ("first", "replayed"):
            a, b = _solve(off, pb), _solve(on, pb)
            _same(a, b, f"pcg miss {k}")


def test_non_finite_start_is_the_same_error(dbg):
    import sfmba
    pb = sfmba.make_problem(3, 8, 20, seed=0)
    x = pb.x0.copy()
    x[0] = np.nan
    off, on = dbg()
    texts = []
    for b in (off, on):
        with pytest.raises(ValueError, match="not finite") as err:
            _solve(b, pb, x0=x)
        texts.append(str(err.value))
    assert texts[0] == texts[1] == "Residuals are not finite in the initial point."
    _same(_solve(off, pb), _solve(on, pb), "solve after the error")        # the handles stay usable


def test_second_solve_from_another_start_right_away(dbg, be):
    """The staging buffer and the copy stream are re-used at once by the next solve on the handle."""
    import sfmba
    for name, pb in (("cfg3", sfmba.make_config("cfg3")), ("cfg4", sfmba.make_config("cfg4"))):
        other = pb.x0 + 1e-3 * np.cos(np.arange(pb.x0.size))
        off, on = dbg()
        _solve(off, pb), _solve(on, pb)
        a, b = _solve(off, pb, x0=other), _solve(on, pb, x0=other)
        _same(a, b, f"{name} second start")
        _same(_solve(be(False), pb, x0=other), b, f"{name} second start against a fresh handle")
        assert not np.array_equal(b[0].x, other)
