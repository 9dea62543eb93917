"""Pin the CPU oracle against fixtures captured from the reference itself (tools/gen_golden.py).

The reference holds no tests for the BA path, so these captures -- the reference's
``compute_residuals`` / ``create_sparsity_matrix`` outputs and scipy runs driven with the kwargs of
/root/reference/sfm_lite/sfm.py:266-268 -- are what pins the oracle.
"""
import json
import os

import numpy as np
import pytest

from oracle import ba_oracle as orc
from sfmba.synthetic import make_problem
from conftest import GOLDEN


def _cases(name):
    g = np.load(os.path.join(GOLDEN, name))
    return g, int(g["n_cases"])


def test_residuals_match_reference_outputs():
    g, n = _cases("residual_cases.npz")
    assert n >= 10
    for k in range(n):
        pre = f"c{k:02d}_"
        C, P, N = (int(v) for v in g[pre + "dims"])
        args = (C, P, g[pre + "ci"], g[pre + "pi"], g[pre + "uv"], g[pre + "K"])
        ref = g[pre + "r"]
        tol = 1e-12 * max(1.0, float(np.abs(ref).max()))      # <=1e-12 relative
        r_vec = orc.compute_residuals(g[pre + "x"], *args)
        r_loop = orc.compute_residuals_loop(g[pre + "x"], *args)
        assert r_vec.shape == ref.shape == (2 * N,)
        assert np.abs(r_vec - ref).max() <= tol, str(g[pre + "tag"])
        assert np.abs(r_loop - ref).max() <= tol, str(g[pre + "tag"])


def test_rodrigues_matches_scipy_capture():
    g = np.load(os.path.join(GOLDEN, "pack_cases.npz"))
    R = orc.rodrigues(g["w"])
    assert np.abs(R - g["R"]).max() < 1e-15 * 4
    for k in range(len(g["w"])):
        back = orc.rotvec_from_matrix(g["R"][k])
        # near pi the log is ill-conditioned (sqrt(eps)); elsewhere full precision
        tol = 1e-7 if np.linalg.norm(g["w"][k]) > 3.1 else 1e-12
        assert np.abs(back - g["rotvec_from_matrix"][k]).max() < tol


def test_sparsity_pattern_matches_reference():
    g = np.load(os.path.join(GOLDEN, "sparsity_cases.npz"))
    C, P, N = (int(v) for v in g["dims"])
    for tag in ("free", "fixed"):
        indptr, indices = orc.create_sparsity_pattern(C, P, N, g["ci"], g["pi"],
                                                      fixed_camera_indices=tuple(g[tag + "_fixed"]))
        assert np.array_equal(indptr, g[tag + "_indptr"])
        assert np.array_equal(indices, g[tag + "_indices"])
        assert tuple(g[tag + "_shape"]) == (2 * N, 6 * C + 3 * P)
        assert np.all(g[tag + "_data"] == 1)


def test_analytic_jacobian_vs_reference_finite_differences():
    g, n = _cases("jacobian_fd_cases.npz")
    for k in range(n):
        pre = f"j{k}_"
        C, P, N = (int(v) for v in g[pre + "dims"])
        pb = make_problem(C, P, N, seed=int(g[pre + "seed"]))
        assert np.array_equal(pb.x0, g[pre + "x"])
        r, Jc, Jp = orc.jacobian_blocks(pb.x0, *pb.args)
        J = orc.jacobian_csr(Jc, Jp, C, P, pb.camera_indices, pb.point_indices).toarray()
        scale = np.abs(g[pre + "J3"]).max()
        assert np.abs(J - g[pre + "J3"]).max() / scale < 1e-8      # 3-point FD of the reference
        assert np.abs(J - g[pre + "J2"]).max() / scale < 1e-5      # the 2-point scheme scipy uses


def test_jacobian_small_angle_branch_is_continuous():
    pb = make_problem(3, 8, 20, seed=0)
    x = pb.x0.copy()
    u = np.array([0.6, -0.64, 0.48])
    outs = []
    for th in (0.9e-4, 1.1e-4, 0.29, 0.31):
        x[0:3] = th * u
        outs.append(orc.jacobian_blocks(x, *pb.args)[1])
    assert np.abs(outs[0] - outs[1]).max() / np.abs(outs[0]).max() < 1e-4
    assert np.abs(outs[2] - outs[3]).max() / np.abs(outs[2]).max() < 0.2


def test_trf_schur_reaches_scipy_minimum_on_tiny_problems():
    """A5-A9: our TRF restatement (exact Schur step) vs recorded scipy outcomes on identical inputs.
    Stated tolerance: final RMSE within 1e-6 px of scipy's; our cost may only be lower (scipy stops in
    its slow tail, optimality 1e-1, ours converges to <1e-3)."""
    g, n = _cases("lsq_tiny_cases.npz")
    for k in range(n):
        pre = f"l{k}_"
        C, P, N = (int(v) for v in g[pre + "dims"])
        pb = make_problem(C, P, N, seed=int(g[pre + "seed"]))
        status, nfev, njev, cost, rmse, opt = g[pre + "summary"]
        for lin in ("dense", "pcg"):
            res = orc.trf_schur(pb.x0, *pb.args, ftol=1e-10, linear=lin, pcg_tol=1e-6)
            my_rmse = float(np.sqrt(np.mean(res.fun ** 2)))
            assert res.status in (1, 2, 3, 4)
            assert abs(my_rmse - rmse) < 1e-6
            assert res.cost <= cost * (1 + 1e-9)
            assert res.nfev <= nfev
            # per-observation residual vectors agree closely as well
            assert np.abs(res.fun - g[pre + "fun"]).max() < 5e-2


def test_unobserved_camera_and_point_match_scipy():
    """Zero Jacobian columns (a camera and a point without observations): scipy's x_scale='jac' maps
    them to scale 1 and never moves them; so does the restatement."""
    from sfmba.synthetic import drop_observations
    g = np.load(os.path.join(GOLDEN, "lsq_tiny_cases.npz"))
    pb = drop_observations(make_problem(5, 40, 200, seed=9), cameras=(3,), points=(7,))
    assert np.array_equal(pb.x0, g["gaps_x0"])
    status, nfev, njev, cost, rmse, opt = g["gaps_summary"]
    res = orc.trf_schur(pb.x0, *pb.args, ftol=1e-10, linear="pcg", pcg_tol=1e-3)
    assert abs(float(np.sqrt(np.mean(res.fun ** 2))) - rmse) < 1e-6 and res.cost <= cost * (1 + 1e-9)
    for sl in (slice(18, 24), slice(30 + 21, 30 + 24)):
        assert np.array_equal(res.x[sl], pb.x0[sl]) and np.array_equal(g["gaps_x"][sl], pb.x0[sl])


def test_ring_scene_large_rotations_match_scipy():
    """Cameras on a ring (rotation vectors up to pi) inside a full solve, against scipy's result."""
    from sfmba.synthetic import make_ring_problem
    g = np.load(os.path.join(GOLDEN, "lsq_tiny_cases.npz"))
    pb = make_ring_problem(12, 150, 900, seed=1)
    assert np.array_equal(pb.x0, g["ring_x0"])
    status, nfev, njev, cost, rmse, opt = g["ring_summary"]
    res = orc.trf_schur(pb.x0, *pb.args, ftol=1e-10, linear="pcg", pcg_tol=1e-3)
    assert abs(float(np.sqrt(np.mean(res.fun ** 2))) - rmse) < 1e-6 and res.cost <= cost * (1 + 1e-9)
    assert np.abs(res.fun - g["ring_fun"]).max() < 5e-2


def test_solver_settings_of_the_hip_path_reach_scipys_answer():
    """The restatement with the settings the HIP path ships -- Schur-diagonal preconditioner, adaptive forcing term
    (1e-2 ... 0.1), or, for few cameras, the diagonal blocks of the formed matrix and a fixed 1e-3 -- against scipy's
    recorded results on the tiny problems and the ring; the exact-block preconditioner equals the per-observation one
    when no (camera, point) pair is observed twice."""
    from sfmba.synthetic import make_ring_problem
    g = np.load(os.path.join(GOLDEN, "lsq_tiny_cases.npz"))
    for k in range(int(g["n_cases"])):
        pre = f"l{k}_"
        C, P, N = (int(v) for v in g[pre + "dims"])
        pb = make_problem(C, P, N, seed=int(g[pre + "seed"]))
        status, nfev, njev, cost, rmse, opt = g[pre + "summary"]
        for kw in (dict(pcg_tol=1e-2, pcg_tol_max=0.1, precond="schur"), dict(pcg_tol=1e-3, precond="schur_exact")):
            res = orc.trf_schur(pb.x0, *pb.args, ftol=1e-10, linear="pcg", **kw)
            assert res.status in (1, 2, 3, 4), kw
            assert abs(float(np.sqrt(np.mean(res.fun ** 2))) - rmse) < 1e-6 and res.cost <= cost * (1 + 1e-9), kw
    pb = make_ring_problem(12, 150, 900, seed=1)
    key = pb.camera_indices.astype(np.int64) * pb.n_points + pb.point_indices
    if len(np.unique(key)) == len(key):                    # no duplicated pair: the two preconditioners coincide
        a = orc.trf_schur(pb.x0, *pb.args, ftol=1e-10, linear="pcg", pcg_tol=1e-3, precond="schur", max_nfev=4)
        b = orc.trf_schur(pb.x0, *pb.args, ftol=1e-10, linear="pcg", pcg_tol=1e-3, precond="schur_exact", max_nfev=4)
        assert np.abs(a.x - b.x).max() <= 1e-9 * np.abs(a.x).max()
    with pytest.raises(ValueError):
        orc.trf_schur(pb.x0, *pb.args, ftol=1e-10, linear="pcg", pcg_tol=1e-3, precond="nope", max_nfev=2)


def test_trf_schur_cfg2_matches_recorded_scipy_run():
    path = os.path.join(GOLDEN, "scipy_cfg2_run.json")
    if not os.path.exists(path):
        pytest.skip("scipy cfg2 capture not generated")
    rec = json.load(open(path))
    pb = make_problem(11, 3000, 10000, seed=0)
    r0 = orc.compute_residuals(pb.x0, *pb.args)
    assert abs(float(np.sqrt(np.mean(r0 ** 2))) - rec["rmse0"]) < 1e-9
    res = orc.trf_schur(pb.x0, *pb.args, ftol=1e-10, linear="pcg", pcg_tol=1e-6)
    my_rmse = float(np.sqrt(np.mean(res.fun ** 2)))
    assert abs(my_rmse - rec["rmse"]) < 1e-6
    assert res.cost <= rec["cost"] * (1 + 1e-9)


def test_pack_unpack_round_trip():
    g = np.load(os.path.join(GOLDEN, "pack_cases.npz"))
    H = g["H"][4:10]                       # generic rotations
    registered = [True, False, True, True, False, True]
    X3d = np.arange(15, dtype=np.float64).reshape(5, 3)
    obs = [(0, 0, (10, 20)), (0, 2, (11, 21)), (1, 3, (5, 6)), (3, 5, (7, 8)), (4, 0, (1, 2))]
    x0, nc, npnt, ci, pi, uv, cmap = orc.pack_problem(H, registered, X3d, obs)
    assert nc == 4 and npnt == 5 and cmap == {0: 0, 2: 1, 3: 2, 5: 3}
    assert np.array_equal(ci, [0, 1, 2, 3, 0]) and np.array_equal(pi, [0, 0, 1, 3, 4])
    assert uv.shape == (5, 2) and uv.dtype.kind == "i"
    for cam_id, n in cmap.items():
        assert np.allclose(x0[6 * n:6 * n + 3], g["rotvec_from_matrix"][4 + cam_id], atol=1e-12)
        assert np.array_equal(x0[6 * n + 3:6 * n + 6], H[cam_id][:3, 3])
    H2, X2 = orc.unpack_result(x0, nc, npnt, cmap, H)
    for k in range(6):
        assert np.allclose(H2[k], H[k], atol=1e-12)
    assert np.array_equal(X2, X3d)


def test_growing_reconstruction_fixture_and_oracle_on_its_first_stages():
    """tests/golden/scipy_growing_run.json (scipy + the reference's residual on a 2 -> 11 camera growing reconstruction,
    /root/reference/sfm_lite/sfm.py:59-71): the stage structure regenerates from the seeded generator, and the oracle,
    started from scipy's recorded x0 of a stage, reaches scipy's RMSE (1e-6 px) with a cost not above scipy's."""
    import json
    import sfmba
    from sfmba.synthetic import growing_reconstruction, make_problem
    path = os.path.join(GOLDEN, "scipy_growing_run.json")
    if not os.path.exists(path):
        pytest.skip("scipy_growing_run.json not generated")
    rec = json.load(open(path))
    arrs = np.load(os.path.join(GOLDEN, "scipy_growing_x.npz"))
    base = rec["base"]
    pb = make_problem(base["n_cameras"], base["n_points"], base["n_obs"], seed=base["seed"])
    stages = list(growing_reconstruction(pb, rec["order"]))
    assert len(stages) == len(rec["stages"]) == pb.n_cameras - 1
    for k, (st, g) in enumerate(zip(stages, rec["stages"])):
        assert (sum(st["registered"]), len(st["cloud"]), len(st["observations"])) == (g["n_cameras"], g["n_points"], g["n_obs"])
        obs = st["observations"]
        assert all(obs[i][0] <= obs[i + 1][0] for i in range(len(obs) - 1))          # point-major, as Graph.pt3ds_pt2ds
        assert g["status"] > 0 and g["rmse"] < 0.5 < g["rmse0"]
        if k > 1:
            continue                                                                   # (oracle runs: the two smallest stages)
        reg = [c for c in range(pb.n_cameras) if st["registered"][c]]
        cmap = {c: i for i, c in enumerate(reg)}
        ci = np.array([cmap[o[1]] for o in obs])
        pi = np.array([o[0] for o in obs])
        uv = np.array([o[2] for o in obs])
        x0 = arrs[f"s{k:02d}_x0"]
        assert x0.shape == (6 * g["n_cameras"] + 3 * g["n_points"],)
        r0 = orc.compute_residuals(x0, g["n_cameras"], g["n_points"], ci, pi, uv, pb.K)
        assert abs(np.sqrt(np.mean(r0 ** 2)) - g["rmse0"]) < 1e-9
        res = orc.trf_schur(x0, g["n_cameras"], g["n_points"], ci, pi, uv, pb.K, ftol=1e-10, linear="pcg", pcg_tol=1e-3,
                            precond="schur_exact")
        assert res.status > 0
        assert abs(np.sqrt(np.mean(res.fun ** 2)) - g["rmse"]) < 1e-6 and res.cost <= g["cost"] * (1 + 1e-9)


def test_similarity_alignment_undoes_a_gauge_transformation_exactly():
    """The residual is invariant under X -> s R X + t, T -> s R T + t, R_c -> R_c R^T (no camera is held, REF
    bundle_adjustment.py:6): similarity_align must find that map and parameter_distance then reads zero."""
    pb = make_problem(6, 60, 400, seed=12)
    C, P = 6, 60
    rng = np.random.default_rng(3)
    s, t = 1.37, rng.normal(size=3)
    R = orc.rodrigues(rng.normal(size=3))
    cams = pb.x0[:6 * C].reshape(C, 6)
    moved = pb.x0.copy()
    mc = moved[:6 * C].reshape(C, 6)
    for c in range(C):
        mc[c, :3] = orc.rotvec_from_matrix(orc.rodrigues(cams[c, :3]) @ R.T)
        mc[c, 3:] = s * R @ cams[c, 3:] + t
    moved[6 * C:] = (s * pb.x0[6 * C:].reshape(P, 3) @ R.T + t).ravel()
    assert np.abs(orc.compute_residuals(moved, *pb.args) - orc.compute_residuals(pb.x0, *pb.args)).max() < 1e-8
    mv = orc.multi_view_points(C, P, pb.camera_indices, pb.point_indices)
    back, (s2, R2, t2) = orc.similarity_align(moved, pb.x0, C, P, fit_points=mv)
    assert abs(s2 * s - 1.0) < 1e-12 and np.abs(R2 @ R - np.eye(3)).max() < 1e-12
    d = orc.parameter_distance(back, pb.x0, C, P, points=mv)
    assert d["points_max"] < 1e-11 and d["centres_max"] < 1e-11 and d["rot_deg_max"] < 1e-9
    # a point seen by one camera only is not counted
    pi = pb.point_indices.copy()
    ci = pb.camera_indices.copy()
    ci[pi == 5] = 2
    assert not orc.multi_view_points(C, P, ci, pi)[5] and mv[5]


def test_recorded_parameter_bounds_are_the_oracles_distance_to_scipy():
    """tests/golden/param_bounds.json (tools/gen_golden.py --params) is what the GPU tests allow the HIP path (times two):
    re-measured here on the tiny cases, and the SceauxCastle-scale numbers DESIGN.md quotes are in it."""
    rows = {(r["case"], r["settings"]): r for r in json.load(open(os.path.join(GOLDEN, "param_bounds.json")))["rows"]}
    g, n = _cases("lsq_tiny_cases.npz")
    for k in range(n):
        pre = f"l{k}_"
        C, P, N = (int(v) for v in g[pre + "dims"])
        pb = make_problem(C, P, N, seed=int(g[pre + "seed"]))
        o = orc.trf_schur(pb.x0, *pb.args, ftol=1e-10, linear="pcg", pcg_tol=1e-3, precond="schur_exact")
        mv = orc.multi_view_points(C, P, pb.camera_indices, pb.point_indices)
        xa, _ = orc.similarity_align(o.x, g[pre + "x"], C, P, fit_points=mv)
        d = orc.parameter_distance(xa, g[pre + "x"], C, P, points=mv)
        rec = rows[(f"tiny{k}_{C}_{P}_{N}", "dense")]
        for key in ("points_rms", "points_max", "centres_max", "rot_deg_max"):
            assert abs(d[key] - rec[key]) <= 1e-6 * rec[key] + 1e-12, (k, key)
    c2 = rows[("cfg2_11_3000_10000", "dense")]
    assert c2["points_rms"] < 1e-4 and c2["points_max"] < 1e-3 and c2["centres_max"] < 3e-4 and c2["rot_deg_max"] < 1e-3
    assert c2["fun_max"] < 3e-3 and c2["points_compared"] == 2649
    assert len([r for r in rows if r[0].startswith("growing_stage")]) == 10


def test_held_cameras_oracle_against_scipys_capture():
    """fixed_camera_indices (REF bundle_adjustment.py:6,13-14) through scipy (tools/gen_golden.py --fixed): the held
    cameras do not move -- in scipy's capture (<= 1e-12: LSMR leaves rounding noise in the empty columns) and, exactly,
    in the oracle -- and the oracle's minimum is not above the cost scipy stops at (scipy's finite differences perturb a
    held camera together with point columns that share its rows, so its Jacobian is off there and it stalls)."""
    g, n = _cases("lsq_fixed_cases.npz")
    assert n == 3
    for k in range(n):
        pre = f"f{k}_"
        C, P, N = (int(v) for v in g[pre + "dims"])
        pb = make_problem(C, P, N, seed=int(g[pre + "seed"]))
        fixed = tuple(int(c) for c in g[pre + "fixed"])
        x0, xs = g[pre + "x0"], g[pre + "x"]
        o = orc.trf_schur(x0, *pb.args, ftol=1e-10, fixed_cameras=fixed, linear="dense")
        for c in fixed:
            assert np.abs(xs[6 * c:6 * c + 6] - x0[6 * c:6 * c + 6]).max() < 1e-12
            assert np.array_equal(o.x[6 * c:6 * c + 6], x0[6 * c:6 * c + 6])
            assert not np.any(o.grad[6 * c:6 * c + 6])
        assert o.status in (2, 3, 4) and o.cost <= float(g[pre + "summary"][3]) * (1 + 1e-9)
        free = orc.trf_schur(x0, *pb.args, ftol=1e-10, linear="dense")
        assert free.cost <= o.cost * (1 + 1e-9)                  # holding cameras can only cost


def test_recorded_shard_runs_decide_nothing_near_a_tie():
    """tests/golden/oracle_cfg4_shard8.json / oracle_cfg5_shard8.json (tools/gen_golden.py --shard NAME 8): the oracle's run
    of rank 0's share of an 8-way sharding, which the GPU tests hold the sharded solver forms to COUNT FOR COUNT.  That is
    only fair where none of the oracle's own stop / continue decisions is near a tie: every recorded ratio
    actual_reduction / (ftol cost) and step_norm / (xtol (xtol + |x|)) -- the operands of the oracle's termination test,
    which stops below 1 -- lies outside [0.5, 2] (nearest: ftol 2.35 / 0.35, xtol 9.7 / 0.10), and the decisions they
    imply are the recorded status and iteration count.  From the files alone."""
    want = {"cfg4": (1000, 12518, 125000, 4, 7, [1, 2, 5, 6, 6, 6]), "cfg5": (5000, 125089, 1250002, 2, 6, [1, 2, 5, 6, 6])}
    for name, (C, P, N, status, nfev, pcg) in want.items():
        with open(os.path.join(GOLDEN, f"oracle_{name}_shard8.json")) as f:
            rec = json.load(f)
        whole = json.load(open(os.path.join(GOLDEN, f"oracle_{name}.json")))
        assert set(whole) <= set(rec) and rec["config"] == whole["config"] and rec["oracle_settings"] == whole["oracle_settings"]
        assert rec["shard"] == dict(rank=0, world=8, n_points=P, n_obs=N) and rec["config"]["n_cameras"] == C
        assert (rec["status"], rec["nfev"], rec["njev"], rec["pcg_iterations"]) == (status, nfev, nfev, pcg)
        fr, xr = rec["ftol_ratio_per_iteration"], rec["xtol_ratio_per_iteration"]
        assert len(fr) == len(xr) == len(pcg) == len(rec["cost_per_iteration"]) - 1
        for r in fr + xr:
            assert np.isfinite(r) and r >= 0 and not (0.5 <= r <= 2.0), (name, r)
        assert all(f > 2.0 and x > 2.0 for f, x in zip(fr[:-1], xr[:-1]))          # every step but the last: continue
        assert {(True, True): 4, (True, False): 2, (False, True): 3}[(fr[-1] < 0.5, xr[-1] < 0.5)] == status
        # the ftol ratio again from the recorded costs (every step of these runs was accepted: nfev == njev)
        cost = rec["cost_per_iteration"]
        assert cost[0] == rec["cost0"] and cost[-1] == rec["cost"]
        for k in range(len(fr) - 2):             # (the last steps' reductions are below the costs' last digits)
            assert abs((cost[k] - cost[k + 1]) / (rec["config"]["ftol"] * cost[k]) - fr[k]) <= 1e-6 * fr[k]


def test_oracle_history_carries_the_operands_of_its_termination_test():
    """history[k] of trf_schur: `reduction`, `step_norm` and `x_norm` of the step INTO iterate k, cost of iterate k --
    what tools/gen_golden.py --shard turns into the recorded ratios.  x_norm is |x| of the iterate the step was taken
    from; the ratios of the last step reproduce the status."""
    pb = make_problem(6, 60, 400, seed=12)
    o = orc.trf_schur(pb.x0, *pb.args, ftol=1e-10, linear="pcg", pcg_tol=1e-2, pcg_tol_max=0.1, precond="schur")
    h = o.history
    assert h[0]["x_norm"] is None and h[0]["reduction"] is None
    assert abs(h[1]["x_norm"] - np.linalg.norm(pb.x0)) <= 1e-14 * np.linalg.norm(pb.x0)
    assert all(h[k]["x_norm"] > 0 for k in range(1, len(h)))
    f_ok = h[-1]["reduction"] < 1e-10 * h[-2]["cost"]
    x_ok = h[-1]["step_norm"] < 1e-8 * (1e-8 + h[-1]["x_norm"])
    assert o.status == (4 if f_ok and x_ok else 2 if f_ok else 3 if x_ok else None)
    for k in range(1, len(h) - 1):
        assert not (h[k]["reduction"] < 1e-10 * h[k - 1]["cost"]) and not (h[k]["step_norm"] < 1e-8 * (1e-8 + h[k]["x_norm"]))
