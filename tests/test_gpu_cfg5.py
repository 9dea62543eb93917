"""BASELINE.json configs[4] at full size on one GPU: 5000 cameras / 1M points / 10M observations, fp32 storage of
the per-observation streams with fp64 arithmetic and accumulation (the per-GPU share on 8 GPUs is 1/8 of the
observations; the camera-side sizes, which decide operand placement, are the same).

At this camera count the camera table of K1 no longer fits the LDS (its rows are fetched from L2), pass A of the Schur
product recomputes its blocks from a table R | T | a' | u_T that k_rc_table writes to global memory, and the PCG update is
a kernel of its own.  In fp32-storage mode the product inside the PCG is the MIXED-PRECISION one configs[4] names: fp32
operands (camera rows, point records), fp64 arithmetic and accumulation -- within 1e-7 of the exact product (bound in the
test: 1e-6), PCG iterations count for count those of the recorded fp64 oracle run; with fp64 storage, or behind debug
option pcg_mixed = 0, the product is exact fp64 (no stored fp32 block is ever applied).
Checked: kernel parity against the oracle on a 200k-observation slice of the same problem, size-independent properties
at full size, the full solves against the recorded oracle run (tests/golden/oracle_cfg5.json), and that the solve is
reproducible: same input, same iteration counts, same bits.
"""
import json
import os

from conftest import GOLDEN
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cfg5():
    import sfmba
    return sfmba.make_config("cfg5")


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(1e-300, np.abs(np.asarray(b)).max()))


def _upper(M):
    iu = np.triu_indices(M.shape[1])
    return M[:, iu[0], iu[1]]


def test_cfg5_slice_parity_vs_oracle(cfg5):
    """First 20 000 points of the cfg5 problem with all their observations (~200k) and all 5000 cameras: the
    same operand placements as the full problem, at a size the oracle finishes in seconds."""
    import sfmba
    from oracle import ba_oracle as orc
    pb = cfg5
    C, Ps = pb.n_cameras, 20000
    n = int(np.searchsorted(pb.point_indices, Ps, side="left"))
    assert 150000 < n < 250000
    args = (C, Ps, pb.camera_indices[:n], pb.point_indices[:n], pb.points_2d[:n], pb.K)
    x = np.concatenate([pb.x0[:6 * C], pb.x0[6 * C:6 * C + 3 * Ps]])
    r_o, Jc_o, Jp_o = orc.jacobian_blocks(x, *args)
    nb = orc.normal_blocks(r_o, Jc_o, Jp_o, C, Ps, args[2], args[3])
    for bits in (64, 32):
        be = sfmba.Backend(0)
        try:
            be.set_precision(bits)
            be.set_problem(*args)
            r, Jc, Jp = be.residual_jacobian(x)
            tol_store = 1e-11 if bits == 64 else 1e-6          # fp32 storage: one rounding of the stored value
            assert np.abs(r - r_o.ravel()).max() <= tol_store * max(3000.0, np.abs(r_o).max())
            assert _rel(Jc, Jc_o) < tol_store and _rel(Jp, Jp_o) < tol_store
            # the normal-equation blocks are recomputed in fp64 in BOTH modes: the gradient is exact
            U, V, gc, gp = be.normal_blocks(x)
            assert _rel(U, _upper(nb.U)) < 1e-11 and _rel(V, _upper(nb.V)) < 1e-11
            assert _rel(gc, nb.gc) < 1e-10 and _rel(gp, nb.gp) < 1e-10
            # implicit Schur product: both passes recompute their blocks in fp64 from the camera table and the points,
            # in both storage modes (the form that applies the stored fp32 blocks survives only behind the debug
            # option sweep_rc = 0, checked below with its own, looser bound)
            rng = np.random.default_rng(1)
            dc = 1e-3 * np.einsum("cii->ci", nb.U) + 1e-6
            dp = 1e-3 * np.einsum("pii->pi", nb.V) + 1e-6
            v = rng.normal(size=6 * C)
            y = be.schur_matvec(x, dc, dp, v)
            Vd = nb.V.copy()
            Vd[:, np.arange(3), np.arange(3)] += dp
            vc = v.reshape(C, 6)
            yy = np.zeros((Ps, 3))
            np.add.at(yy, args[3], np.einsum("nij,ni->nj", nb.W, vc[args[2]]))
            z = np.einsum("pij,pj->pi", np.linalg.inv(Vd), yy)
            ref = np.einsum("cij,cj->ci", nb.U, vc) + dc * vc
            np.add.at(ref, args[2], -np.einsum("nij,nj->ni", nb.W, z[args[3]]))
            w = rng.normal(size=6 * C)
            yw = be.schur_matvec(x, dc, dp, w)
            if bits == 64:
                assert _rel(y, ref.ravel()) < 1e-9
                assert abs(v @ yw - w @ y) <= 1e-10 * abs(v @ yw)
            else:
                # fp32 operands (R, T - o, X - o, a', u_T, z), fp64 arithmetic: measured 1e-7 of the exact product and
                # symmetric to 1e-7 (both passes see the same rounded operands; z and a' are rounded themselves)
                assert 1e-12 < _rel(y, ref.ravel()) < 1e-6
                assert abs(v @ yw - w @ y) <= 1e-6 * abs(v @ yw)
                # ... and the exact fp64 product stays available in this storage mode
                be.debug_option("pcg_mixed", 0)
                be.set_problem(*args)
                y = be.schur_matvec(x, dc, dp, v)
                yw = be.schur_matvec(x, dc, dp, w)
                assert _rel(y, ref.ravel()) < 1e-9
                assert abs(v @ yw - w @ y) <= 1e-10 * abs(v @ yw)
        finally:
            be.close()
    # the debug form sweep_rc = 0 in fp32-storage mode really applies rounded blocks (pass A the stored ones, pass B its
    # own rounded the same way): one fp32 rounding per entry, and still the product of ONE symmetric matrix
    be = sfmba.Backend(0)
    try:
        be.debug_option("sweep_rc", 0)
        be.set_precision(32)
        be.set_problem(*args)
        y = be.schur_matvec(x, dc, dp, v)
        yw = be.schur_matvec(x, dc, dp, w)
        assert 1e-12 < _rel(y, ref.ravel()) < 2e-6
        assert abs(v @ yw - w @ y) <= 1e-10 * abs(v @ yw)
    finally:
        be.close()


def test_cfg5_full_size_fp32_storage(cfg5):
    import sfmba
    pb = cfg5
    C, P, N = pb.n_cameras, pb.n_points, pb.n_obs
    assert (C, P, N) == (5000, 1000000, 10000000)
    be = sfmba.Backend(0)
    try:
        be.set_precision(32)
        be.set_problem(*pb.args)
        rng = np.random.default_rng(0)
        # (1) the truth reproduces the integer pixels to within truncation + noise (+ one fp32 rounding of r)
        r_true = be.residuals(pb.x_true)
        assert np.abs(r_true).max() < 1.0 + 6 * 0.5
        # (2) the gradient (exact fp64 in this mode too) against a directional finite difference of the cost,
        #     the cost taken from a solve capped at its initial evaluation (summed in fp64 before r is rounded)
        U, V, gc, gp = be.normal_blocks(pb.x0)
        gvec = np.concatenate([gc.ravel(), gp.ravel()])
        d = rng.normal(size=gvec.shape)
        d /= np.linalg.norm(d)
        opt = be.default_options()
        opt.ftol, opt.max_nfev = 1e-10, 1

        def cost_at(x):
            return be.solve(x, opt, want_fun=False, want_grad=False)[1].cost0
        eps = 1e-4
        fd = (cost_at(pb.x0 + eps * d) - cost_at(pb.x0 - eps * d)) / (2 * eps)
        assert abs(fd - gvec @ d) <= 1e-5 * abs(fd)
        # (3) the implicit Schur complement is linear, symmetric and positive
        dc = 1e-3 * U[:, [0, 6, 11, 15, 18, 20]] + 1e-6
        dp = 1e-3 * V[:, [0, 3, 5]] + 1e-6
        v, w = rng.normal(size=6 * C), rng.normal(size=6 * C)
        Sv, Sw = be.schur_matvec(pb.x0, dc, dp, v), be.schur_matvec(pb.x0, dc, dp, w)
        Svw = be.schur_matvec(pb.x0, dc, dp, 2.0 * v - 3.0 * w)
        assert _rel(Svw, 2.0 * Sv - 3.0 * Sw) < 1e-6                  # (fp32 operands: a', u_T, z are rounded per product)
        assert abs(v @ Sw - w @ Sv) <= 1e-6 * abs(v @ Sw) and v @ Sv > 0
        # (4) full solves with the reference's tolerance: converge to the noise floor of the generator, and
        #     back-to-back solves from the same x0 are THE SAME solve -- iteration counts equal, every bit of x
        #     equal (no atomics anywhere; the gradient does not carry fp32 noise, so ftol = 1e-10 terminates the
        #     fp32-storage solve where it terminates the fp64 one)
        opt = be.default_options()
        opt.ftol = 1e-10
        runs = [be.solve(pb.x0, opt, want_fun=False, want_grad=False) for _ in range(3)]
        x0_, r0 = runs[0][0], runs[0][1]
        assert r0.status > 0 and r0.cost < r0.cost0 and 0.3 < r0.rmse < 0.7
        for x_, r_, _, _ in runs[1:]:
            assert ((r_.iterations, r_.nfev, r_.njev, r_.pcg_iterations, r_.status) ==
                    (r0.iterations, r0.nfev, r0.njev, r0.pcg_iterations, r0.status))
            assert r_.cost == r0.cost and np.array_equal(x_, x0_)
        r_fin = be.residuals(x0_)
        assert abs(0.5 * np.sum(r_fin ** 2) - r0.cost) <= 1e-6 * r0.cost      # r is stored in fp32
        hist32 = be.pcg_history()
    finally:
        be.close()
    rec = None
    if os.path.exists(os.path.join(GOLDEN, "oracle_cfg5.json")):
        # the recorded fp64 run of the oracle (tools/gen_golden.py --full cfg5, build container): the fp32-storage solve
        # takes the same outer iterations, evaluations and PCG iterations; its steps come from fp32-stored blocks
        # (k_jdot, k_backsub), so its cost agrees to 1e-8 rather than 1e-9
        with open(os.path.join(GOLDEN, "oracle_cfg5.json")) as f:
            rec = json.load(f)
        assert (int(r0.status), int(r0.nfev), int(r0.njev)) == (rec["status"], rec["nfev"], rec["njev"])
        assert hist32 == rec["pcg_iterations"]
        assert abs(r0.cost - rec["cost"]) <= 1e-8 * rec["cost"] and abs(r0.rmse - rec["rmse"]) <= 1e-8
    # fp64 storage on the same problem: same basin, same iteration count (+-1), RMSE within 1e-6 px
    be = sfmba.Backend(0)
    try:
        be.set_problem(*pb.args)
        opt = be.default_options()
        opt.ftol = 1e-10
        x64, r64, _, _ = be.solve(pb.x0, opt, want_fun=False, want_grad=False)
        assert r64.status > 0 and abs(r64.rmse - r0.rmse) < 1e-6
        assert abs(int(r64.iterations) - int(r0.iterations)) <= 1
        assert abs(r64.cost - r0.cost) <= 1e-8 * r64.cost
        if rec is not None:                   # fp64 storage: the oracle's run to 1e-9, count for count
            assert (int(r64.status), int(r64.nfev), int(r64.njev)) == (rec["status"], rec["nfev"], rec["njev"])
            assert be.pcg_history() == rec["pcg_iterations"]
            assert abs(r64.cost0 - rec["cost0"]) <= 1e-12 * rec["cost0"]
            assert abs(r64.cost - rec["cost"]) <= 1e-9 * rec["cost"] and abs(r64.rmse - rec["rmse"]) <= 1e-9
            ck = rec["x_checksum"]
            assert abs(np.sum(x64) - ck["sum"]) <= 1e-8 * ck["abs_sum"]
    finally:
        be.close()


# ---- the sharded forms at 5000 cameras: rank 0's share of an 8-way sharding, a world of one ---------------------------

def _check_fp32_against_record(be, pb, rec, measured):
    """fp32 storage against the recorded fp64 oracle run: counts and PCG history equal, cost 1e-8 relative, rmse 1e-8 --
    the bounds test_cfg5_full_size_fp32_storage states for the same comparison."""
    opt = be.default_options()
    opt.ftol = rec["config"]["ftol"]
    x, res, _, _ = be.solve(pb.x0, opt, want_fun=False, want_grad=False)
    measured.update(status=int(res.status), nfev=int(res.nfev), njev=int(res.njev), pcg=be.pcg_history(),
                    cost_rel=abs(res.cost - rec["cost"]) / rec["cost"], rmse_abs=abs(res.rmse - rec["rmse"]))
    print("measured against the record:", measured)
    assert (int(res.status), int(res.nfev), int(res.njev)) == (rec["status"], rec["nfev"], rec["njev"])
    assert be.pcg_history() == rec["pcg_iterations"] and int(res.pcg_iterations) == sum(rec["pcg_iterations"])
    assert abs(res.cost - rec["cost"]) <= 1e-8 * rec["cost"] and abs(res.rmse - rec["rmse"]) <= 1e-8
    return x, res


def test_cfg5_shard_of_8_sharded_forms_world_of_one_vs_recorded_oracle_and_blocks(cfg5):
    """Rank 0's share of an 8-way sharding of cfg5 (5000 / 125089 / 1250002: what one of eight GPUs holds) on a handle
    sharded with a world of one (test_gpu_fullsize.sharded_world_of_one).  At 5000 cameras the sharded iteration takes
    forms no small test reaches together: pass A's table in global memory, the PCG update a kernel of its own, with
    fp32 storage the mixed-precision product, and the per-camera exchange inside K3 / the right-hand-side pass / pass B.
    Held to the oracle's recorded fp64 run of the SAME shard (oracle_cfg5_shard8.json, ``tools/gen_golden.py --shard
    cfg5 8``; tests/test_oracle_golden.py asserts that none of its decisions is near a tie), each with the in-kernel
    exchange and with the collectives as launches of their own (pcg_inline = 0):
    * fp32 storage, mixed product as shipped: counts and PCG history equal, cost 1e-8 relative, rmse 1e-8;
    * fp64 storage: the same and the checksums, cost 1e-9.
    The same shard on a plain handle: counts and history equal, cost within 1e-9 (fp64; fp32 storage against fp32
    storage: the 1e-8 of that mode).  The exchanged quantities at x0 against the oracle's blocks of the shard:
    [U | g_c], V, g_p (recomputed in fp64 in both storage modes) 1e-11 / 1e-10, S v 1e-9 in fp64 and behind
    pcg_mixed = 0, the mixed product inside (1e-12, 1e-6) and symmetric to 1e-6.
    Sharded against plain: the in-kernel form equals the plain handle's solve to the BIT in both storage modes (asserted);
    the form with the collectives as launches orders the four per-camera PCG scalar sums differently (pcg_tail_camera:
    one thread, index order; pass B's tail: a wave reduction) -- cost 3.3e-16 (fp64) / 6.6e-16 (fp32) apart, x 4.8e-12 /
    1.3e-6 (fp32-stored blocks in the step).
    Measured on an MI355X: fp32 storage cost 1.2e-15 (bound 1e-8), rmse 2.2e-16 (1e-8); fp64 storage cost0 2.1e-16 (1e-12),
    cost 1.2e-15 (1e-9), rmse 2.2e-16 (1e-9), checksums 0 (1e-8); 181 vs 220 launches per solve in both modes; U 1.3e-15,
    V 3.9e-16 (1e-11), g_c 1.9e-15, g_p 5.6e-15 (1e-10); S v 1.8e-15 in fp64 and behind pcg_mixed = 0 (1e-9), symmetric
    to 0 (1e-10); the mixed product 1.1e-7 (inside 1e-12 ... 1e-6), symmetric to 4.1e-9 (1e-6).
    Wall time: 2 s of the 25 s the sharded-form tests add to ``pytest -m gpu`` (test_gpu_fullsize.py has the account)."""
    from oracle import ba_oracle as orc
    from test_gpu_fullsize import (exchanged_quantities_against_oracle, plain_solve, rank0_shard,
                                   sharded_solves_against_record, sharded_world_of_one)
    with open(os.path.join(GOLDEN, "oracle_cfg5_shard8.json")) as f:
        rec = json.load(f)
    pb = rank0_shard(cfg5, 8)
    assert (pb.n_cameras, pb.n_points, pb.n_obs) == (rec["config"]["n_cameras"], rec["shard"]["n_points"], rec["shard"]["n_obs"])
    for bits, check, tol in ((32, _check_fp32_against_record, 1e-8), (64, None, 1e-9)):
        runs = sharded_solves_against_record(pb, rec, bits=bits, check=check)
        xp, rp, hp = plain_solve(pb, rec, bits=bits)
        for form, (x, res) in runs.items():
            same = np.array_equal(x, xp) and res.cost == rp.cost
            print(f"fp{bits} {form} vs plain handle: cost differs by {abs(res.cost - rp.cost) / rp.cost:.3e}, x by {np.abs(x - xp).max():.3e}, "
                  f"bitwise equal: {same}")
            assert (int(res.status), int(res.nfev), int(res.njev)) == (int(rp.status), int(rp.nfev), int(rp.njev))
            assert hp == rec["pcg_iterations"]
            assert abs(res.cost - rp.cost) <= tol * rp.cost
            assert same or form != "inline"              # the in-kernel form IS the plain handle's, to the bit
    r_o, Jc_o, Jp_o = orc.jacobian_blocks(pb.x0, *pb.args)
    nb = orc.normal_blocks(r_o, Jc_o, Jp_o, pb.n_cameras, pb.n_points, pb.camera_indices, pb.point_indices)
    del r_o, Jc_o, Jp_o
    for bits, debug, mixed in ((64, (), False), (32, (), True), (32, (("pcg_mixed", 0),), False)):
        with sharded_world_of_one(pb, bits=bits, debug=debug) as handle:
            exchanged_quantities_against_oracle(handle, pb, nb, mixed=mixed)
