"""Full-solve parity at the sizes the bench quotes, a growing reconstruction against recorded scipy runs, and a problem
read from a BAL file -- all through the C-ABI on the GPU.

* BASELINE.json configs[3] (cfg4, 1000 / 100k / 1M): the recorded run of the oracle with the shipped solver settings
  (tests/golden/oracle_cfg4.json, written by ``tools/gen_golden.py --full cfg4`` in the build container; the oracle
  needs a minute there, scipy itself ~20 min per iteration).  Status, nfev, njev and the PCG
  iterations of every outer iteration must be EQUAL, the cost within 1e-9 relative.
* the reference's real call pattern (/root/reference/sfm_lite/sfm.py:59-71: BA after every registration, warm-started
  from the previous result): ``tests/golden/scipy_growing_run.json`` holds scipy.optimize.least_squares driving the
  reference's own compute_residuals through a 2 -> 11 camera reconstruction cut from the SceauxCastle-scale
  synthetic; one handle goes through the same stages via ``sfmba.apply_bundle_adjustment``.
* a BAL text file written in the test, ``read_bal`` -> ``least_squares`` against the oracle.
* the observation-SHARDED forms of the iteration at 1000 cameras, on a handle "sharded with a world of one"
  (``sharded_world_of_one``: transport registered, direct link attached to the rank's own buffer -- the per-camera sums
  of K3, the right-hand-side pass and pass B go through cam_exchange_value, the scalars through k_p2p_allreduce): the
  whole cfg4 problem against oracle_cfg4.json, rank 0's share of an 8-way sharding against oracle_cfg4_shard8.json
  (``tools/gen_golden.py --shard cfg4 8``), and the exchanged quantities themselves -- [U | g_c] and S v -- against the
  oracle's blocks of the same shard.  (tests/test_gpu_cfg5.py: the same at 5000 cameras.)
"""
import contextlib
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu


def _golden(name):
    path = os.path.join(GOLDEN, name)
    if not os.path.exists(path):
        pytest.skip(f"{name} not generated")
    with open(path) as f:
        return json.load(f)


def _record(name):
    """A recorded oracle run the sharded-form tests are held to: committed, so a missing file is an error, not a skip."""
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def check_against_recorded_oracle(be, pb, rec, cost_tol=1e-9, measured=None):
    """One solve with the reference's ftol on handle `be` (problem already set) against a recorded oracle run.
    `measured` (a dict): takes the figures the bounds are compared with, printed before anything is asserted."""
    opt = be.default_options()
    opt.ftol = rec["config"]["ftol"]
    x, res, _, _ = be.solve(pb.x0, opt, want_fun=False, want_grad=False)
    if measured is not None:
        measured.update(status=int(res.status), nfev=int(res.nfev), njev=int(res.njev), pcg=be.pcg_history(),
                        cost0_rel=abs(res.cost0 - rec["cost0"]) / rec["cost0"], cost_rel=abs(res.cost - rec["cost"]) / rec["cost"],
                        rmse_abs=abs(res.rmse - rec["rmse"]), sum_rel=abs(np.sum(x) - rec["x_checksum"]["sum"]) / rec["x_checksum"]["abs_sum"])
        print("measured against the record:", measured)
    assert (int(res.status), int(res.nfev), int(res.njev)) == (rec["status"], rec["nfev"], rec["njev"])
    assert be.pcg_history() == rec["pcg_iterations"]
    assert int(res.pcg_iterations) == sum(rec["pcg_iterations"])
    assert abs(res.cost0 - rec["cost0"]) <= 1e-12 * rec["cost0"]
    assert abs(res.cost - rec["cost"]) <= cost_tol * rec["cost"]
    assert abs(res.rmse - rec["rmse"]) <= 1e-9
    # the parameters themselves: the sums the oracle recorded (a similarity gauge is free, but both runs take the same
    # steps from the same start, so they agree far beyond the 1e-6 the RMSE target asks for)
    ck = rec["x_checksum"]
    assert abs(np.sum(x) - ck["sum"]) <= 1e-8 * ck["abs_sum"]
    assert abs(np.sum(x[:6 * pb.n_cameras]) - ck["cams_sum"]) <= 1e-8 * ck["abs_sum"]
    return x, res


def test_cfg4_full_solve_equals_the_recorded_oracle_run():
    import sfmba
    rec = _golden("oracle_cfg4.json")
    pb = sfmba.make_config("cfg4")
    assert (pb.n_cameras, pb.n_points, pb.n_obs) == (rec["config"]["n_cameras"], rec["config"]["n_points"], rec["config"]["n_obs"])
    be = sfmba.Backend(0)
    try:
        be.set_problem(*pb.args)
        x, res = check_against_recorded_oracle(be, pb, rec)
        # and the first solve on a fresh handle (no PCG record to replay) equals the second (record replayed)
        x2, res2 = check_against_recorded_oracle(be, pb, rec)
        assert np.array_equal(x, x2) and res.cost == res2.cost
    finally:
        be.close()


# ---- the sharded forms of the iteration on ONE device: a world of one -------------------------------------------------

def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(1e-300, np.abs(np.asarray(b)).max()))


def _upper(M):
    iu = np.triu_indices(M.shape[1])
    return M[:, iu[0], iu[1]]


def rank0_shard(pb, world):
    from sfmba import dist as sdist
    return sdist.shard_problem(pb, sdist.partition_points(pb.point_indices, pb.n_points, world)[0])


@contextlib.contextmanager
def sharded_world_of_one(pb, bits=64, debug=(), attach=True):
    """-> (handle, fallback transport, link): a handle that runs the SHARDED forms of the iteration without a peer, as
    ``bench.py --force-exchange`` sets one up -- an in-process torch.distributed group (rank 0 of 1), the callback
    transport over it as the fallback, and the direct link attached to the rank's own staging buffer
    (``DirectLink(allow_single=True)``), kernels and collectives on one torch stream.  With a world of one
    cam_exchange_value has no peer to wait for: nothing here can block on an exchange.  A link that does not attach is a
    failure.  `attach` = False leaves the link out (to see by hand that the checks of ``solve_sharded`` then trip)."""
    import socket
    import torch
    import torch.distributed as td
    import sfmba
    from sfmba import dist as sdist
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    torch.cuda.set_device(0)
    td.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
    be = link = None
    try:
        be = sfmba.Backend(0)
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            be.set_stream(stream.cuda_stream)
            be.set_precision(bits)
            for name, value in debug:
                be.debug_option(name, value)
            be.set_problem(*pb.args)
            ex = sdist.Exchange(be, n_obs_local=pb.n_obs, device="cuda")
            assert ex.n_obs_total == pb.n_obs
            if attach:
                link = sdist.DirectLink(be, allow_single=True)
                assert link.active, "the direct link did not attach to the rank's own buffer (mapping or self-test failed)"
            yield be, ex, link
            torch.cuda.synchronize()
    finally:
        if link is not None:
            link.close()
        if be is not None:
            be.close()
        td.destroy_process_group()


def solve_sharded(handle, solve):
    """Runs `solve(be)` on a handle of ``sharded_world_of_one`` and asserts that the SHARDED path is what ran: the link
    is attached, direct collectives and per-camera exchanges were enqueued, the fallback transport served none of them.
    -> (what `solve` returned, kernel launches it enqueued)."""
    be, ex, link = handle
    assert link is not None and link.active, "no direct link: the solve would run the collective launches over the fallback"
    p0, e0, (l0, c0) = be.p2p_calls(), ex.n_calls, be.counters()
    out = solve(be)
    l1, c1 = be.counters()
    print(f"sharded path: {be.p2p_calls() - p0} direct calls, {c1 - c0} collectives, {l1 - l0} launches, fallback calls {ex.n_calls - e0}")
    assert be.p2p_calls() > p0, "no collective went over the direct link"
    assert ex.n_calls == e0, "the fallback transport served a collective of the solve"
    assert c1 > c0, "the solve enqueued no collective"
    return out, l1 - l0


def sharded_solves_against_record(pb, rec, bits=64, check=None, attach=True):
    """The shared body of the world-of-one solve tests: `pb` solved with the sharded forms, with the per-camera exchange
    inside the producing kernels (pcg_inline at its default) and with the collectives as launches of their own
    (pcg_inline = 0), each held to the recorded oracle run `rec` by `check(be, pb, rec, measured)`; the default form
    must need fewer launches.  -> {form: (x, result)}."""
    check = check or (lambda be, pb_, rec_, m: check_against_recorded_oracle(be, pb_, rec_, measured=m))
    runs, launches = {}, {}
    for form, debug in (("inline", ()), ("launches", (("pcg_inline", 0),))):
        with sharded_world_of_one(pb, bits=bits, debug=debug, attach=attach) as handle:
            runs[form], launches[form] = solve_sharded(handle, lambda be: check(be, pb, rec, {"form": form, "bits": bits}))
    print("launches per solve:", launches)
    assert launches["inline"] < launches["launches"], launches       # the exchange really ran inside the producing kernels
    return runs


def plain_solve(pb, rec, bits=64):
    """The same problem on a plain handle (no transport): -> (x, result, PCG history)."""
    import sfmba
    be = sfmba.Backend(0)
    try:
        be.set_precision(bits)
        be.set_problem(*pb.args)
        opt = be.default_options()
        opt.ftol = rec["config"]["ftol"]
        x, res, _, _ = be.solve(pb.x0, opt, want_fun=False, want_grad=False)
        return x, res, be.pcg_history()
    finally:
        be.close()


def explicit_schur_product(nb, args, dc, dp, v):
    """U v + dc v - W (V + diag dp)^-1 W^T v from the oracle's blocks `nb` of the problem `args`."""
    C, P, ci, pi = args[0], args[1], np.asarray(args[2]), np.asarray(args[3])
    Vd = nb.V.copy()
    Vd[:, np.arange(3), np.arange(3)] += np.asarray(dp).reshape(P, 3)
    vc = np.asarray(v).reshape(C, 6)
    yy = np.zeros((P, 3))
    np.add.at(yy, pi, np.einsum("nij,ni->nj", nb.W, vc[ci]))
    z = np.einsum("pij,pj->pi", np.linalg.inv(Vd), yy)
    ref = np.einsum("cij,cj->ci", nb.U, vc) + np.asarray(dc).reshape(C, 6) * vc
    np.add.at(ref, ci, -np.einsum("nij,nj->ni", nb.W, z[pi]))
    return ref.ravel()


def exchanged_quantities_against_oracle(handle, pb, nb, mixed=False):
    """What the sharded forms exchange -- [U | g_c] (K3 with the in-kernel exchange: cam_inline holds on `handle`) and
    S v (schur_product_standalone + one 6 C collective) -- on a world-of-one handle against the oracle's blocks `nb` of
    the same problem.  Bounds: the ones tests/test_gpu_cfg5.py::test_cfg5_slice_parity_vs_oracle states for the same
    quantities.  -> the measured errors."""
    import torch.distributed as td
    be, ex, link = handle
    C = pb.n_cameras
    (U, V, gc, gp), _ = solve_sharded(handle, lambda b: b.normal_blocks(pb.x0))
    err = dict(U=_rel(U, _upper(nb.U)), V=_rel(V, _upper(nb.V)), gc=_rel(gc, nb.gc), gp=_rel(gp, nb.gp))
    rng = np.random.default_rng(1)
    dc = 1e-3 * np.einsum("cii->ci", nb.U) + 1e-6
    dp = 1e-3 * np.einsum("pii->pi", nb.V) + 1e-6
    v, w = rng.normal(size=6 * C), rng.normal(size=6 * C)
    ref = explicit_schur_product(nb, pb.args, dc, dp, v)
    td.barrier()           # K3 owns ONE slot set: a grid-wide collective (here: the barrier) between two of its launches
    y, _ = solve_sharded(handle, lambda b: b.schur_matvec(pb.x0, dc, dp, v))
    td.barrier()
    yw = be.schur_matvec(pb.x0, dc, dp, w)
    err.update(y=_rel(y, ref), sym=abs(v @ yw - w @ y) / abs(v @ yw))
    print("exchanged quantities against the oracle:", err)
    assert err["U"] < 1e-11 and err["V"] < 1e-11 and err["gc"] < 1e-10 and err["gp"] < 1e-10
    if mixed:
        assert 1e-12 < err["y"] < 1e-6 and err["sym"] <= 1e-6
    else:
        assert err["y"] < 1e-9 and err["sym"] <= 1e-10
    return err


def test_cfg4_sharded_forms_world_of_one_equal_the_recorded_oracle_run():
    """The WHOLE cfg4 problem through the sharded forms at 1000 cameras -- the fused PCG with its per-camera tail in pass
    B and the exchange in K3 / the right-hand-side pass / pass B (default), and the same with every collective a launch
    of its own (pcg_inline = 0) -- held to oracle_cfg4.json exactly as the plain solve is: status, nfev, njev and PCG
    history equal, cost within 1e-9, checksums within 1e-8 abs_sum.
    Measured on an MI355X, both forms alike: cost0 2.6e-16 (bound 1e-12), cost 6.1e-16 (1e-9), rmse 3.3e-16 (1e-9), checksums
    0 (1e-8); 126 launches per solve with the in-kernel exchange, 174 with pcg_inline = 0.
    Wall time: the tests on the sharded forms (the three world-of-one tests here and in tests/test_gpu_cfg5.py, and the
    three multi-process ones in tests/test_gpu_parity.py) add 25 s to ``pytest -m gpu`` -- 60 tests in 101 s against the
    parent commit's 54 in 76 s, same machine, same session.  The multi-process cases dominate (128 / 129 edge 13 s,
    exchanged quantities on 2-3 ranks 9 s, 2-process cfg4 3 s: process start-up); the world-of-one tests take 3 s
    (cfg4) and 2 s (cfg5 / 8)."""
    import sfmba
    rec = _record("oracle_cfg4.json")
    pb = sfmba.make_config("cfg4")
    assert (pb.n_cameras, pb.n_points, pb.n_obs) == (rec["config"]["n_cameras"], rec["config"]["n_points"], rec["config"]["n_obs"])
    sharded_solves_against_record(pb, rec)


def test_cfg4_shard_of_8_sharded_forms_world_of_one_vs_recorded_oracle_and_blocks():
    """Rank 0's share of an 8-way sharding of cfg4 (1000 / 12518 / 125000: what one of eight GPUs holds), solved with the
    sharded forms (in-kernel exchange; collectives as launches) and held to the oracle's recorded run of the SAME shard
    (oracle_cfg4_shard8.json; tests/test_oracle_golden.py asserts that none of that run's decisions is near a tie): counts
    and PCG history equal, cost 1e-9, checksums.  The same shard on a plain handle (no transport): counts and history
    equal, cost within 1e-9.  And the exchanged quantities themselves at x0 -- [U | g_c] from K3 with the in-kernel
    exchange, S v from the standalone product + its collective -- against the oracle's blocks of the shard.
    Sharded against plain: the in-kernel form IS the plain handle's iteration -- a world-of-one exchange adds nothing -- and is
    asserted equal to it to the BIT (x and cost).  The form with the collectives as launches is not: its per-camera PCG
    bookkeeping runs behind the reduction (k_p2p_pcg / k_pcg_tail -> pcg_tail_camera), where one thread adds the six
    terms of a camera's dot products (u.Su, s.u, s.Minv s, r.u) in index order, while the tail inside pass B adds them
    with a wave reduction: the four PCG scalar sums are ordered differently (cost 1.5e-15, x 8.7e-13 apart; bound 1e-9).
    Measured on an MI355X: cost0 2.6e-16 (1e-12), cost 2.1e-15 / 6.3e-16 (1e-9), rmse 3.3e-16 (1e-9), checksums 5.9e-16
    (1e-8); 154 vs 216 launches per solve; U 8.0e-16, V 2.6e-16 (1e-11), g_c 2.7e-15, g_p 4.8e-15 (1e-10), S v 1.5e-15
    (1e-9), symmetry 8.1e-16 (1e-10)."""
    import sfmba
    from oracle import ba_oracle as orc
    rec = _record("oracle_cfg4_shard8.json")
    pb = rank0_shard(sfmba.make_config("cfg4"), 8)
    assert (pb.n_cameras, pb.n_points, pb.n_obs) == (rec["config"]["n_cameras"], rec["shard"]["n_points"], rec["shard"]["n_obs"])
    runs = sharded_solves_against_record(pb, rec)
    xp, rp, hp = plain_solve(pb, rec)
    for form, (x, res) in runs.items():
        same = np.array_equal(x, xp) and res.cost == rp.cost
        print(f"{form} vs plain handle: cost differs by {abs(res.cost - rp.cost) / rp.cost:.3e}, x by {np.abs(x - xp).max():.3e}, bitwise equal: {same}")
        assert (int(res.status), int(res.nfev), int(res.njev)) == (int(rp.status), int(rp.nfev), int(rp.njev))
        assert hp == rec["pcg_iterations"]
        assert abs(res.cost - rp.cost) <= 1e-9 * rp.cost
        assert same or form != "inline"                  # the in-kernel form IS the plain handle's, to the bit
    r_o, Jc_o, Jp_o = orc.jacobian_blocks(pb.x0, *pb.args)
    nb = orc.normal_blocks(r_o, Jc_o, Jp_o, pb.n_cameras, pb.n_points, pb.camera_indices, pb.point_indices)
    with sharded_world_of_one(pb) as handle:
        exchanged_quantities_against_oracle(handle, pb, nb)


def test_growing_reconstruction_matches_recorded_scipy_runs():
    """Stage k: nodes order[:k+2] registered, cloud = every point two registered nodes see.  scipy's result per stage
    was recorded with the reference's residual and kwargs (sfm.py:266-268); here ONE handle (the calling thread's)
    runs the same chain through apply_bundle_adjustment, each stage warm-started from its own previous result as
    sfm.py:271-281 writes it back.  Bar (north_star): RMSE within 1e-6 px of scipy's at every stage, cost not above
    scipy's (the Schur step converges further than scipy's LSMR iterates do before ftol stops them)."""
    import sfmba
    rec = _golden("scipy_growing_run.json")
    arrs = np.load(os.path.join(GOLDEN, "scipy_growing_x.npz"))
    base = rec["base"]
    pb = sfmba.make_problem(base["n_cameras"], base["n_points"], base["n_obs"], seed=base["seed"])
    C = pb.n_cameras
    cams0 = pb.x0[:6 * C].reshape(C, 6)
    pts0 = pb.x0[6 * C:].reshape(-1, 3)
    from sfmba.api import _matrix_from_rotvec
    H = [np.eye(4) for _ in range(C)]
    X3d = np.zeros((0, 3))
    be = sfmba.get_backend(0)
    reused_any = False
    for k, st in enumerate(sfmba.growing_reconstruction(pb, rec["order"])):
        g = rec["stages"][k]
        for c in st["new_camera"]:
            H[c][:3, :3] = _matrix_from_rotvec(cams0[c, :3])
            H[c][:3, 3] = cams0[c, 3:]
        X3d = np.vstack([X3d, pts0[st["cloud"][len(X3d):]]])
        assert (sum(st["registered"]), len(X3d), len(st["observations"])) == (g["n_cameras"], g["n_points"], g["n_obs"])
        H, X3d, res = sfmba.apply_bundle_adjustment(H, st["registered"], X3d, st["observations"], pb.K, tol=rec["ftol"],
                                                    verbose=0)
        reused_any |= be.problem_reuse()[0] > 0
        assert res.success
        # (stage inputs differ from scipy's: no camera is fixed, so the two solvers drift differently along the
        # 7-dimensional gauge, while a new camera / new points enter in absolute coordinates -- the minimum they
        # converge to is the same; the replay from scipy's own x0 below compares like with like)
        assert abs(res.rmse - g["rmse"]) < 1e-6, (k, res.rmse, g["rmse"])
        assert res.cost <= g["cost"] * (1 + 1e-9), (k, res.cost, g["cost"])
        # identical inputs: scipy's own x0 of the stage (its previous results written back) instead of ours
        x0s = arrs[f"s{k:02d}_x0"]
        n_cam, n_pts = g["n_cameras"], g["n_points"]
        _, _, _, ci, pi, uv, _ = sfmba.pack_cameras_points(H, st["registered"], X3d, st["observations"])
        r2 = sfmba.least_squares(sfmba.compute_residuals, x0s, x_scale="jac", ftol=rec["ftol"], method="trf",
                                 args=(n_cam, n_pts, ci, pi, uv, pb.K))
        assert abs(r2.rmse0 - g["rmse0"]) < 1e-9 and abs(r2.rmse - g["rmse"]) < 1e-6 and r2.cost <= g["cost"] * (1 + 1e-9)
    assert k + 1 == len(rec["stages"]) == C - 1


def test_bal_file_problem_solves_like_the_oracle(tmp_path):
    """A file in the published BAL text format (camera-major observation order, P = R X + t, p = -P / P.z, one focal
    length, no distortion) written here; read_bal maps it onto the reference's model with K = diag(-f, -f, 1) and
    point-major order.  The HIP residual at x0 is BAL's own reprojection error; the solve equals the oracle's."""
    import sfmba
    from oracle import ba_oracle as orc
    rng = np.random.default_rng(5)
    C, P, f0 = 7, 160, 1100.0
    rot = rng.normal(0, 0.15, (C, 3))
    t = rng.normal(0, 0.4, (C, 3)) + np.array([0.0, 0.0, -8.0])          # BAL cameras look down -z
    X = rng.normal(0, 1.0, (P, 3))
    obs = [(c, p) for c in range(C) for p in range(P) if rng.random() < 0.6]          # camera-major, as BAL files are
    lines = [f"{C} {P} {len(obs)}"]
    px_file = []
    for c, p in obs:
        Pc = orc.rodrigues(rot[c]) @ X[p] + t[c]
        px = -f0 * Pc[:2] / Pc[2] + rng.normal(0, 0.4, 2)
        px_file.append(px)
        lines.append(f"{c} {p} {float(px[0])!r} {float(px[1])!r}")
    rot0 = rot + rng.normal(0, 0.01, rot.shape)                           # the file holds a perturbed start
    t0 = t + rng.normal(0, 0.02, t.shape)
    X0 = X + rng.normal(0, 0.02, X.shape)
    for c in range(C):
        lines += [repr(float(v)) for v in (*rot0[c], *t0[c], f0, 0.0, 0.0)]
    for p in range(P):
        lines += [repr(float(v)) for v in X0[p]]
    path = tmp_path / "problem-7-160-pre.txt"
    path.write_text("\n".join(lines) + "\n")
    x0, args, info = sfmba.read_bal(path)
    assert info["exact"] and args[5][0, 0] == -f0 and np.all(np.diff(args[3]) >= 0)
    # residual at x0 == BAL's reprojection error of the file's own parameters, observation by observation
    r = sfmba.compute_residuals(x0, *args).reshape(-1, 2)
    want = np.empty_like(r)
    for k, j in enumerate(info["file_order"]):
        c, p = obs[j]
        Pc = orc.rodrigues(rot0[c]) @ X0[p] + t0[c]
        want[k] = -f0 * Pc[:2] / Pc[2] - px_file[j]
    assert np.abs(r - want).max() < 1e-9
    # the solve: 7 cameras -> the in-LDS PCG; and the implicit-product path on the same file
    res = sfmba.least_squares(sfmba.compute_residuals, x0, x_scale="jac", ftol=1e-10, method="trf", args=args)
    o = orc.trf_schur(x0, *args, ftol=1e-10, linear="pcg", pcg_tol=1e-3, precond="schur_exact")
    assert (res.status, res.nfev, res.njev) == (o.status, o.nfev, o.njev)
    assert abs(res.cost - o.cost) <= 1e-8 * o.cost and res.cost < 0.05 * res.cost0
    be = sfmba.Backend(0)
    try:
        be.debug_option("dense", 0)
        res2 = sfmba.least_squares(sfmba.compute_residuals, x0, x_scale="jac", ftol=1e-10, method="trf", args=args, backend=be)
        o2 = orc.trf_schur(x0, *args, ftol=1e-10, linear="pcg", pcg_tol=1e-2, pcg_tol_max=0.1, precond="schur")
        assert (res2.status, res2.nfev, res2.njev) == (o2.status, o2.nfev, o2.njev)
        assert abs(res2.cost - o2.cost) <= 1e-8 * o2.cost
    finally:
        be.close()
    # written back and read again: the same problem
    out = tmp_path / "solved.txt.gz"
    sfmba.write_bal(out, res.x, *args)
    x1, args1, _ = sfmba.read_bal(out)
    r1 = sfmba.compute_residuals(x1, *args1)
    assert abs(0.5 * np.sum(r1 ** 2) - res.cost) <= 1e-9 * res.cost
