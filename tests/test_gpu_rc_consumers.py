"""k_jdot and k_backsub in row form (debug option rc_consumers; DESIGN.md sections 5 and 12): the two products with the whole
Jacobian taken from pass A's LDS camera rows R | T | a' | u_T and the point instead of from the stored blocks.
The forms table takes the row form from 65536 observations on; the problems here are smaller (tests stay quick), so
they ask for it with rc_consumers = 1 -- "wherever it is legal" -- and check through the form query that it ran.
Entry by entry against extended-precision numpy (both forms), whole solves against the stored-Jacobian form and the
oracle, the FinalUpdate hand-over of replayed records, and the sharded forms on a world of one."""
import numpy as np
import pytest

from entry_bounds import CHOL_ROUNDINGS, EPS, LD, T1_ROUNDINGS, T_ROUNDINGS, _cross_abs, _inv3, _row_form_abs, _run_roundings  # noqa: F401
from step_products_ref import _Case, _check_entries, rc_hand_built as _hand_built  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def orc():
    from oracle import ba_oracle
    return ba_oracle


# ---- 1. entries against extended precision ---------------------------------------------------------------------------
# Roundings on the longest path of an entry, counted from ba_kernels.hpp with every multiplication and addition as one
# rounding (the compiler contracts some pairs into FMAs: fewer, never more).  The camera table R | T | w b c and the
# fetched residuals are inputs of both forms, of K1 and of the reference alike and are not counted.
#   row form (rc_row_products):  v = X - T 1;  q = R v 3;  p = K q 3;  iz 1;  pk 1;  b = (K - pk K) iz 3;  j = b R 3:  15 for j;
#       a' (rc_put_au): w x u 2, w x (w x u) 2, u - b c + cc d 3, g = v x a' + u_T 3: 10 < 15;  t = -(j . g) 3:  18 for t
#       t1 = t + j . w_p:  19
#   stored form (k_jdot / k_backsub):  t = jc . u, six terms added to 0: 7;  t1 = nine terms: 10
#   y_p = sum of jp^T t: 2 more, then the sum over the run: seg_reduce_serial 7 steps, or (run longer than the window)
#       ceil(L / 64) serial additions and the 6 steps of wave_sum
#   dp = Vinv (-g_p - y): 1 + 3, Vinv by chol3_inverse: 15 on its longest path (inv[0]), on V + diag (1), V and g_p summed
#       over the run by K1 (products 1, the same run sums)
#   t2 = t + jp . dp: 4 more than the later of t and dp
#   sums: products 2, then one addition per window of the lane's range, 6 (wave_sum), 16 (waves of the workgroup), and the
#       workgroups' partial rows
# k is TWICE the count: the reference is formed from the fetched blocks, which carry K1's roundings of the same paths.
# (the constants, _run_roundings, _row_form_abs, _cross_abs and _inv3 live in tests/entry_bounds.py, shared with test_gpu_entries.py;
# _Case, _check_entries and the hand-built problem in tests/step_products_ref.py, shared with test_gpu_step_products.py)


def _both_forms(pb, tag, fixed=(), expect_row_form=1):
    import sfmba
    outs, case = {}, None
    for rc in (0, 1):
        be = sfmba.Backend(0)
        try:
            be.debug_option("dense", 0)
            be.debug_option("rc_consumers", rc)
            be.set_fixed_cameras(fixed)
            be.set_problem(*pb.args)
            assert be.form("rc_cons") == (expect_row_form if rc else 0), tag
            case = case or _Case(be, pb)
            outs[rc] = _check_entries(be, pb, be.form("rc_cons"), case, tag)
        finally:
            be.close()
    return outs


CASES = ("tiny", "medium", "hand_built", "gaps", "held_camera")


@pytest.mark.parametrize("name", CASES)
def test_entries_against_extended_precision(orc, name):
    """t1, sum |t1|^2, dp and the ten sums of sfmba_step_products, stored-Jacobian form and row form, entry by entry within
    k eps sum |terms| of the longdouble value (k and the terms: the comment at the top of this file)."""
    import sfmba
    if name == "tiny":
        pb, fixed = sfmba.make_problem(6, 80, 500, seed=5), ()
    elif name == "medium":
        pb, fixed = sfmba.make_problem(60, 900, 9000, seed=12), ()
    elif name == "hand_built":
        pb, fixed = _hand_built(orc), ()
        L = np.bincount(pb.point_indices, minlength=40)
        assert L.max() == 200 and np.sum(L == 1) >= 3 and np.cumsum(L)[20] == 63 and L[21] > 1
    elif name == "gaps":
        pb, fixed = sfmba.drop_observations(sfmba.make_problem(6, 80, 500, seed=5), cameras=(3,), points=(7,)), ()
    else:
        pb, fixed = sfmba.make_problem(6, 80, 500, seed=5), (2,)
    _both_forms(pb, name, fixed=fixed)


def test_forms_table_at_its_size_and_storage_switches():
    """The default (rc_consumers = -1): the row form from 65536 observations on, not below; never with fp32 storage; and
    rc_consumers = 0 / 1 override the size, not the legality."""
    import sfmba
    be = sfmba.Backend(0)
    try:
        for n_obs, bits, rc, want in ((65535, 64, -1, 0), (65536, 64, -1, 1), (65536, 32, -1, 0), (65536, 32, 1, 0),
                                      (65536, 64, 0, 0), (65535, 64, 1, 1)):
            pb = sfmba.make_problem(40, 8000, n_obs, seed=2)
            be.set_precision(bits)
            be.debug_option("rc_consumers", rc)
            be.set_problem(*pb.args)
            assert be.form("rc_cons") == want, (n_obs, bits, rc)
    finally:
        be.close()


def test_largest_camera_count_of_the_row_form_and_the_first_above(orc):
    """1100 cameras is what pass A's LDS table takes (kRcMaxCams): the row form runs there; at 1101 the table decides for the
    stored-Jacobian readers, whatever rc_consumers asks for, and the default equals rc_consumers = 0 to the bit."""
    import sfmba
    _both_forms(sfmba.make_problem(1100, 1500, 12000, seed=8), "1100 cameras")
    pb = sfmba.make_problem(1101, 1500, 12000, seed=8)
    rng = np.random.default_rng(3)
    sg, dc, diag = rng.normal(size=pb.x0.shape[0]), 1e-2 * rng.normal(size=6 * 1101), rng.uniform(1.0, 2.0, size=3 * 1500)
    outs = {}
    for rc in (-1, 0, 1):
        be = sfmba.Backend(0)
        try:
            be.debug_option("rc_consumers", rc)
            be.set_problem(*pb.args)
            assert be.form("rc_cons") == 0 and be.form("sweep_rc") == 0
            outs[rc] = be.step_products(pb.x0, sg, dc, diag)
        finally:
            be.close()
    for rc in (-1, 1):
        assert all(np.array_equal(outs[rc][k], outs[0][k]) for k in ("t1", "dp", "sums")) and outs[rc]["g11"] == outs[0]["g11"]


# ---- 2. whole solves ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", range(4))
def test_whole_solves_row_form_against_stored_jacobian_form(orc, which):
    """rc_consumers = 0 against the row form (1: these problems are below the size from which it is the default) on ONE
    handle, held to the bounds between two forms of one algorithm (test_fused_pcg_launch_equals_sweep_plus_update); the
    first two problems also against the oracle."""
    import sfmba
    pb = (lambda: sfmba.make_config("cfg2"), lambda: sfmba.make_problem(300, 4000, 30000, seed=3),
          lambda: sfmba.make_problem(6, 80, 500, seed=5, x0_noise=0.2), lambda: sfmba.make_problem(1024, 3000, 20000, seed=8))[which]()
    be = sfmba.Backend(0)
    try:
        be.debug_option("dense", 0)
        runs = []
        for rc in (0, 1):
            be.debug_option("rc_consumers", rc)
            be.set_problem(*pb.args)
            assert be.form("rc_cons") == rc
            opt = be.default_options()
            opt.ftol = 1e-10
            x, res, fun, _ = be.solve(pb.x0, opt)
            runs.append((x, res, fun, be.pcg_history()))
    finally:
        be.close()
    (xa, a, fa, _), (xb, b, fb, _) = runs
    print(f"problem {which}: cost {a.cost!r} / {b.cost!r}, max |dx| {np.abs(xa - xb).max():.3e}, max |dfun| {np.abs(fa - fb).max():.3e}")
    assert (a.nfev, a.pcg_iterations) == (b.nfev, b.pcg_iterations)
    assert abs(a.njev - b.njev) <= 1 and {a.status, b.status} <= {2, 3, 4}
    assert abs(a.cost - b.cost) <= 1e-12 * a.cost
    assert np.abs(xa - xb).max() <= 1e-6 * np.abs(xa).max()
    assert np.abs(fa - fb).max() <= 1e-6
    if which < 2:
        from test_gpu_parity import _oracle_kwargs
        o = orc.trf_schur(pb.x0, *pb.args, ftol=1e-10, **_oracle_kwargs(False))
        assert (b.status, b.nfev, b.njev) == (o.status, o.nfev, o.njev)
        assert abs(b.cost - o.cost) <= 1e-9 * o.cost


# ---- 3. the FinalUpdate hand-over --------------------------------------------------------------------------------------
def test_final_update_in_the_row_form_prologue():
    """Back-to-back solves on one handle replay the PCG record, and the launch of pass A that would only find the solve
    finished is left to k_backsub_rc's prologue (pcg_skip_last at its default); with pcg_skip_last = 0 every launch is
    enqueued.  Exact replays, a record made too short by a tighter pcg_tol and one that is too long: x, nfev, cost and
    the PCG history are those of a fresh handle, to the bit."""
    import sfmba
    pb = sfmba.make_problem(60, 900, 9000, seed=12)
    hist = {}
    for tol in (1e-2, 1e-5):
        fresh = sfmba.Backend(0)
        fresh.debug_option("dense", 0)
        fresh.debug_option("rc_consumers", 1)
        fresh.set_problem(*pb.args)
        assert fresh.form("rc_cons") == 1
        opt = fresh.default_options()
        opt.ftol = 1e-10
        opt.pcg_tol = opt.pcg_tol_max = tol
        x, res, _, _ = fresh.solve(pb.x0, opt)
        hist[tol] = (x, res.nfev, res.cost, fresh.pcg_history())
        fresh.close()
    assert sum(hist[1e-5][3]) > sum(hist[1e-2][3]) + 5
    be = sfmba.Backend(0)
    try:
        be.debug_option("dense", 0)
        be.debug_option("rc_consumers", 1)
        be.set_problem(*pb.args)
        assert be.form("rc_cons") == 1
        opt = be.default_options()
        opt.ftol = 1e-10
        launches = {}
        for skip in (-1, 0):
            be.debug_option("pcg_skip_last", skip)
            for tol in (1e-2, 1e-2, 1e-5, 1e-5, 1e-2):
                opt.pcg_tol = opt.pcg_tol_max = tol
                l0 = be.counters()[0]
                x, res, _, _ = be.solve(pb.x0, opt)
                launches[skip, tol] = be.counters()[0] - l0        # (the last of each tolerance: an exact or too long replay)
                assert np.array_equal(x, hist[tol][0]) and (res.nfev, res.cost) == hist[tol][1:3]
                assert be.pcg_history() == hist[tol][3]
        # the prologue really stood in for launches: two per outer iteration fewer than with every launch enqueued
        assert launches[-1, 1e-5] < launches[0, 1e-5]
    finally:
        be.close()


# ---- 4. the sharded forms on a world of one ------------------------------------------------------------------------------
def test_world_of_one_sharded_path_with_row_form_consumers():
    """The sharded forms of the iteration (collectives over the direct link, per-camera exchanges inside the kernels; the
    non-FinalUpdate prologue of k_backsub_rc on x of the PCG's final set) give the counts of the local form, cost to 1e-9."""
    import sfmba
    from test_gpu_fullsize import sharded_world_of_one, solve_sharded
    pb = sfmba.make_problem(100, 2000, 16000, seed=6)

    def solve(be):
        assert be.form("rc_cons") == 1
        opt = be.default_options()
        opt.ftol = 1e-10
        x, res, _, _ = be.solve(pb.x0, opt, want_fun=False, want_grad=False)
        return x, res, be.pcg_history()

    local = sfmba.Backend(0)
    try:
        local.debug_option("rc_consumers", 1)
        local.set_problem(*pb.args)
        xl, rl, hl = solve(local)
    finally:
        local.close()
    with sharded_world_of_one(pb, debug=(("rc_consumers", 1),)) as handle:
        (xs, rs, hs), _ = solve_sharded(handle, solve)
    assert (rs.status, rs.nfev, rs.njev, rs.pcg_iterations) == (rl.status, rl.nfev, rl.njev, rl.pcg_iterations) and hs == hl
    assert abs(rs.cost - rl.cost) <= 1e-9 * rl.cost
