"""The fp64 row-form kernels take the rows of d r/d X from M = K R (DESIGN.md sections 5 and 12): the camera table keeps a
compact view M | T beside R | T, pass A (k_point_sweep_rc), the exact-block branch of pass B (k_cam_schur), k_jdot_rc and
k_backsub_rc form  p = M v,  j_k = (M_k - (p_k / p_z) M_3) / p_z  from it.

Small problems (about 2000 observations) at the camera counts where the kernels change path: 3 cameras, 64, 1024 (the last
count of the fused PCG prologue, one thread per camera) and 1100 (kRcMaxCams, the last LDS table), each with a point of 200
observations (the long-run path), a run of five that starts on lane 63 of the first 64-observation window, and a camera
whose rotation vector is exactly zero.  The intrinsics are general: unequal focal lengths, skew, a principal point, and in
two cases a third row that is not (0, 0, 1), so that M_3 differs from R_3.

Bounds are those of the existing tests of the same quantities: the product within 1e-9 of the oracle's and symmetric to
1e-10 (tests/test_gpu_parity.py: _matvec_case, test_properties_at_full_size); k_jdot_rc / k_backsub_rc entry by entry within
the rounding counts of tests/test_gpu_rc_consumers.py, and the two forms against each other within the sum of their bounds."""
import numpy as np
import pytest

from entry_bounds import LD
from test_gpu_parity import _matvec_case
from test_gpu_rc_consumers import _Case

pytestmark = pytest.mark.gpu

K_SKEW = np.array([[2905.88, 3.7, 1416.0], [0.0, 2811.4, 1064.0], [0.0, 0.0, 1.0]])
K_ROW3 = np.array([[2905.88, 3.7, 1416.0], [1.3, 2811.4, 1064.0], [1e-3, -2e-3, 0.5]])       # K[2, 2] = 0.5: M_3 != R_3
SHAPES = ((3, K_ROW3), (64, K_SKEW), (1024, K_SKEW), (1100, K_ROW3))


@pytest.fixture(scope="module")
def orc():
    from oracle import ba_oracle
    return ba_oracle


_problems = {}


def _problem(orc, C, K):
    """420 points: 21 of 3 observations (0..62), a run of 5 from lane 63 on, one point of 200, the rest 1..8 each; cameras
    dealt out in turn, so that each of 3 / 64 is seen often and each of 1024 / 1100 once or twice; camera 0 unrotated."""
    if C in _problems:
        return _problems[C]
    import sfmba
    from sfmba.synthetic import BAProblem
    P = 420
    rng = np.random.default_rng(1000 + C)
    counts = np.concatenate([[3] * 21, [5], [200], rng.integers(1, 9, P - 23)])
    pi = np.repeat(np.arange(P, dtype=np.int64), counts)
    N = len(pi)
    ci = (np.arange(N, dtype=np.int64) * 7) % C                  # 7 is coprime to every C here: each camera is seen
    ci[63] = 0                                                   # the straddling run is seen by the unrotated camera too
    base = sfmba.make_problem(C, P, N, seed=C, K=K)
    x_true, x0 = base.x_true.copy(), base.x0.copy()
    x_true[:3] = 0.0
    x0[:3] = 0.0
    args = (C, P, ci, pi, np.zeros((N, 2)), K)
    uv = orc.compute_residuals(x_true, *args).reshape(-1, 2) + rng.normal(0.0, 0.5, (N, 2))
    pb = BAProblem(C, P, ci, pi, uv, K, x0, x_true)
    L = np.bincount(pi, minlength=P)
    assert 1900 <= N <= 2200 and L.max() == 200 and np.cumsum(L)[20] == 63 and L[21] == 5 and len(np.unique(ci)) == C
    _problems[C] = pb
    return pb


@pytest.mark.parametrize("C,K", SHAPES, ids=[str(s[0]) for s in SHAPES])
def test_product_against_the_oracle_and_its_symmetry(orc, C, K):
    """S v of passes A and B against the oracle's blocks, and u . S v = v . S u."""
    import sfmba
    pb = _problem(orc, C, K)
    be = sfmba.Backend(0)
    try:
        be.set_problem(*pb.args)
        assert be.form("sweep_rc") == 1
        r, Jc, Jp = orc.jacobian_blocks(pb.x0, *pb.args)
        nb = orc.normal_blocks(r, Jc, Jp, C, pb.n_points, pb.camera_indices, pb.point_indices)
        _matvec_case(be, orc, pb, nb, seed=C)                    # rel. 1e-9 of the largest entry
        rng = np.random.default_rng(C)
        dc = 1e-3 * np.einsum("cii->ci", nb.U) + 1e-6
        dp = 1e-3 * np.einsum("pii->pi", nb.V) + 1e-6
        u, v = rng.normal(size=6 * C), rng.normal(size=6 * C)
        Su, Sv = be.schur_matvec(pb.x0, dc, dp, u), be.schur_matvec(pb.x0, dc, dp, v)
        print(f"{C} cameras: u.Sv {u @ Sv!r}, v.Su {v @ Su!r}, rel {abs(u @ Sv - v @ Su) / abs(u @ Sv):.3e}")
        assert abs(u @ Sv - v @ Su) <= 1e-10 * abs(u @ Sv)
        assert v @ Sv > 0
    finally:
        be.close()


def _entries_within_bounds(be, pb, form, case, tag):
    """The accuracy assertions of test_gpu_rc_consumers._check_entries, with its bounds: t1, dp and the eleven sums of
    sfmba_step_products against the extended-precision reference.  (That function also asserts that no sum of ITS cases
    cancels -- every bound nine digits below its sum; with 2000 observations sum t1 . t2 of the 1024-camera problem here
    cancels to 1.2e6 of terms three orders larger, which says nothing about the kernels.)"""
    out = be.step_products(pb.x0, case.sg, case.dc, case.diag)
    seen = case.seen
    err_t1 = np.abs(out["t1"].astype(LD) - case.t1)
    err_dp = np.abs(out["dp"].astype(LD) - case.dp)[seen]
    ref, bound = case.sums(out, form)
    got = np.concatenate([[out["g11"]], out["sums"]]).astype(LD)
    err_s = np.abs(got - ref)
    print(f"{tag} form {form}: t1 err/bound {float((err_t1 / case.B_t1[form]).max()):.3f}, "
          f"dp {float((err_dp / case.B_dp[form][seen]).max()):.3f}, "
          f"sums {np.array2string(np.asarray(err_s / bound, dtype=np.float64), precision=3)}")
    assert np.all(np.isfinite(out["t1"])) and np.all(np.isfinite(out["dp"][seen])) and np.all(np.isfinite(got.astype(np.float64)))
    assert np.all(err_t1 <= case.B_t1[form]), tag
    assert np.all(err_dp <= case.B_dp[form][seen]), tag
    assert np.all(err_s <= bound), (tag, err_s / bound)
    # the entries' bounds mean something: nine digits below all but a hundredth of the entries
    assert np.mean(case.B_t1[form] < 1e-9 * np.abs(case.t1)) >= 0.99, tag
    assert np.mean(case.B_dp[form][seen] < 1e-9 * np.abs(case.dp[seen])) >= 0.99, tag
    return out, bound


@pytest.mark.parametrize("C,K", SHAPES, ids=[str(s[0]) for s in SHAPES])
def test_row_form_consumers_against_the_stored_jacobian_forms(orc, C, K):
    """k_jdot_rc and k_backsub_rc (rc_consumers = 1) and the stored-Jacobian forms (0): each within its bound of the
    extended-precision reference (tests/test_gpu_rc_consumers.py), hence within the sum of the two of each other."""
    import sfmba
    pb = _problem(orc, C, K)
    outs, case, sums = {}, None, {}
    for rc in (0, 1):
        be = sfmba.Backend(0)
        try:
            be.debug_option("dense", 0)
            be.debug_option("rc_consumers", rc)
            be.set_problem(*pb.args)
            assert be.form("rc_cons") == rc
            case = case or _Case(be, pb, seed=C)
            outs[rc], sums[rc] = _entries_within_bounds(be, pb, rc, case, f"{C} cameras")
        finally:
            be.close()
    seen = case.seen
    d_t1 = np.abs(outs[1]["t1"].astype(LD) - outs[0]["t1"].astype(LD))
    d_dp = np.abs(outs[1]["dp"].astype(LD) - outs[0]["dp"].astype(LD))[seen]
    got = [np.concatenate([[outs[rc]["g11"]], outs[rc]["sums"]]).astype(LD) for rc in (0, 1)]
    assert np.all(d_t1 <= case.B_t1[0] + case.B_t1[1])
    assert np.all(d_dp <= (case.B_dp[0] + case.B_dp[1])[seen])
    assert np.all(np.abs(got[1] - got[0]) <= sums[0] + sums[1])


def test_second_solve_on_a_handle_sees_fresh_rows(orc):
    """Solve, then solve from another start on the same handle: bitwise what a fresh handle gives from that start.  The
    M | T view is written with every table (upload, trial point); a stale one would move the second solve."""
    import sfmba
    pb = _problem(orc, 64, K_SKEW)
    x0b = pb.x0 + np.random.default_rng(5).normal(0.0, 0.02, pb.x0.shape)

    def run(be, x0):
        opt = be.default_options()
        opt.ftol = 1e-10
        x, res, fun, _ = be.solve(x0, opt)
        return x, fun, (res.status, res.nfev, res.njev, res.pcg_iterations, res.cost), be.pcg_history()

    runs = []
    for first in (pb.x0, None):
        be = sfmba.Backend(0)
        try:
            be.debug_option("dense", 0)                          # the PCG pair, not the dense reduced-camera solve
            be.debug_option("rc_consumers", 1)
            be.set_problem(*pb.args)
            assert be.form("sweep_rc") == 1 and be.form("rc_cons") == 1
            if first is not None:
                a = run(be, first)
                assert a[2][0] > 0 and a[2][3] > 0
            runs.append(run(be, x0b))
        finally:
            be.close()
    (xa, fa, ra, ha), (xb, fb, rb, hb) = runs
    assert ra == rb and ha == hb
    assert np.array_equal(xa, xb) and np.array_equal(fa, fb)
