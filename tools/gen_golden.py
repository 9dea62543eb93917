#!/usr/bin/env python3
"""Generate tests/golden/*.npz by running the REFERENCE's own hot-path module in the build container.

Runs only where /root/reference exists (never on the GPU box).  The reference package itself cannot be
imported (``sfm_lite/__init__.py`` pulls in cv2, which is not installed), but its BA module
``/root/reference/sfm_lite/bundle_adjustment.py`` depends only on numpy + scipy and is loaded by file
path.  Outputs are data only: inputs + the reference's outputs (+ scipy's, driven with the exact kwargs
of /root/reference/sfm_lite/sfm.py:266-268).  No reference source is written anywhere.

    python tools/gen_golden.py            # fast fixtures (seconds)
    python tools/gen_golden.py --cfg2     # also the ~7 min scipy run on the SceauxCastle-scale synthetic
    python tools/gen_golden.py --full cfg4   # oracle.trf_schur with the shipped settings at BASELINE's full size
    python tools/gen_golden.py --full cfg5   #   (cfg4: ~1 min, cfg5: ~15 min and ~25 GB; build container only)
    python tools/gen_golden.py --shard cfg4 8   # the same for rank 0's share of an 8-way sharding (cfg4: seconds,
    python tools/gen_golden.py --shard cfg5 8   #   cfg5: under a minute)
    python tools/gen_golden.py --growing  # scipy + the reference residual on a 2 -> 11 camera growing reconstruction
    python tools/gen_golden.py --fixed    # scipy + the reference's pattern with fixed_camera_indices (seconds)
    python tools/gen_golden.py --triangulate   # the reference's two-view DLT on synthetic pixel pairs, and the bounds of
                                          #   the triangulation tests (seconds)
    python tools/gen_golden.py --params   # gauge-aligned parameter distance oracle <-> scipy on every stored scipy x
                                          #   (re-runs the last growing stage with scipy: ~4 min)
"""
from __future__ import annotations

import argparse
import importlib.util
import io
import json
import os
import re
import sys
import time
from contextlib import redirect_stdout

import numpy as np
from scipy.optimize import least_squares
from scipy.optimize._numdiff import approx_derivative
from scipy.spatial.transform import Rotation as Rot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sfm-python_amd"))
from sfmba.synthetic import drop_observations, make_problem, make_ring_problem  # noqa: E402

REF_BA = "/root/reference/sfm_lite/bundle_adjustment.py"
OUT = os.path.join(ROOT, "tests", "golden")


def load_ref():
    spec = importlib.util.spec_from_file_location("ref_ba", REF_BA)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def residual_cases(ba):
    """Inputs -> reference compute_residuals outputs."""
    out = {}
    n = 0

    def add(tag, x, C, P, ci, pi, uv, K):
        nonlocal n
        r = ba.compute_residuals(np.asarray(x, dtype=np.float64), C, P, ci, pi, uv, K)
        pre = f"c{n:02d}_"
        out[pre + "tag"] = np.array(tag)
        out[pre + "x"] = np.asarray(x, dtype=np.float64)
        out[pre + "dims"] = np.array([C, P, len(ci)], dtype=np.int64)
        out[pre + "ci"] = np.asarray(ci, dtype=np.int64)
        out[pre + "pi"] = np.asarray(pi, dtype=np.int64)
        out[pre + "uv"] = np.asarray(uv)
        out[pre + "K"] = np.asarray(K, dtype=np.float64)
        out[pre + "r"] = r
        n += 1

    for seed in range(3):
        pb = make_problem(3, 8, 20, seed=seed)
        add(f"rand_3_8_20_s{seed}", pb.x0, *pb.args)
        pb = make_problem(4, 30, 120, seed=10 + seed)
        add(f"rand_4_30_120_s{seed}", pb.x0, *pb.args)
    # rotation magnitudes across scipy's Taylor switch (theta <= 1e-3) and large angles
    pb = make_problem(11, 12, 44, seed=5)
    mags = [0.0, 1e-12, 1e-8, 1e-4, 1e-3, 1.1e-3, 0.1, 1.0, 3.0, np.pi, 5.0]
    rng = np.random.default_rng(99)
    x = pb.x0.copy()
    for c, m in enumerate(mags):
        u = rng.normal(size=3)
        u /= np.linalg.norm(u)
        x[6 * c:6 * c + 3] = m * u
    add("theta_sweep", x, *pb.args)
    # K with skew and unequal focal lengths
    Ksk = np.array([[1200.5, 3.25, 640.0], [0.0, 1100.25, 360.5], [0.0, 0.0, 1.0]])
    pb = make_problem(4, 30, 120, seed=21, K=Ksk)
    add("skewK", pb.x0, *pb.args)
    # a fully general 3x3 "K" (utils.py:34 only asserts the shape)
    Kg = np.array([[900.0, 2.0, 500.0], [1.5, 950.0, 400.0], [1e-3, -2e-3, 1.0]])
    pb = make_problem(4, 30, 120, seed=22, K=Kg)
    add("generalK", pb.x0, *pb.args)
    # float observations instead of int64
    pb = make_problem(4, 30, 120, seed=23)
    add("float_uv", pb.x0, pb.n_cameras, pb.n_points, pb.camera_indices, pb.point_indices,
        pb.points_2d.astype(np.float64) + 0.25, pb.K)
    # duplicated (camera, point) pairs (track merging, graph.py:86)
    pb = make_problem(3, 8, 20, seed=24)
    ci = pb.camera_indices.copy()
    ci[1] = ci[0]
    pi = pb.point_indices.copy()
    pi[1] = pi[0]
    add("dup_pairs", pb.x0, 3, 8, ci, pi, pb.points_2d, pb.K)
    # single observation
    pb = make_problem(1, 1, 1, seed=25)
    add("single", pb.x0, *pb.args)
    out["n_cases"] = np.array(n)
    return out


def sparsity_cases(ba):
    """A3: CSR structure of create_sparsity_matrix, with and without fixed cameras."""
    pb = make_problem(4, 10, 30, seed=3)
    out = {"dims": np.array([4, 10, 30]), "ci": pb.camera_indices, "pi": pb.point_indices}
    for tag, fixed in (("free", ()), ("fixed", (0, 2))):
        M = ba.create_sparsity_matrix(4, 10, 30, pb.camera_indices, pb.point_indices,
                                      fixed_camera_indices=fixed).tocsr()
        M.sort_indices()
        out[tag + "_indptr"] = M.indptr.astype(np.int64)
        out[tag + "_indices"] = M.indices.astype(np.int64)
        out[tag + "_data"] = M.data.astype(np.int64)
        out[tag + "_shape"] = np.array(M.shape)
        out[tag + "_fixed"] = np.array(fixed, dtype=np.int64)
    return out


def jacobian_cases(ba):
    """A6: scipy finite differences of the REFERENCE residual (3-point and the 2-point scheme scipy
    actually uses with jac_sparsity)."""
    out = {}
    for k, (C, P, N, seed) in enumerate([(3, 8, 20, 0), (4, 30, 120, 11)]):
        pb = make_problem(C, P, N, seed=seed)
        fun = lambda x: ba.compute_residuals(x, *pb.args)  # noqa: E731
        J3 = approx_derivative(fun, pb.x0, method="3-point")
        S = ba.create_sparsity_matrix(C, P, N, pb.camera_indices, pb.point_indices)
        J2 = approx_derivative(fun, pb.x0, method="2-point", sparsity=S).toarray()
        pre = f"j{k}_"
        out[pre + "dims"] = np.array([C, P, N])
        out[pre + "seed"] = np.array(seed)
        out[pre + "x"] = pb.x0
        out[pre + "J3"] = J3
        out[pre + "J2"] = J2
    out["n_cases"] = np.array(2)
    return out


def lsq_tiny(ba):
    """A5-A9: full scipy runs with the kwargs of sfm.py:266-268 on tiny problems."""
    out = {}
    for k, (C, P, N, seed) in enumerate([(3, 8, 40, 0), (4, 30, 120, 11), (6, 60, 400, 12)]):
        pb = make_problem(C, P, N, seed=seed)
        S = ba.create_sparsity_matrix(C, P, N, pb.camera_indices, pb.point_indices)
        res = least_squares(ba.compute_residuals, pb.x0, jac_sparsity=S, verbose=0, x_scale="jac",
                            ftol=1e-10, method="trf", args=pb.args)
        pre = f"l{k}_"
        out[pre + "dims"] = np.array([C, P, N])
        out[pre + "seed"] = np.array(seed)
        out[pre + "x0"] = pb.x0
        out[pre + "x"] = res.x
        out[pre + "fun"] = res.fun
        out[pre + "summary"] = np.array([res.status, res.nfev, res.njev, res.cost,
                                         np.sqrt(np.mean(res.fun ** 2)), res.optimality])
        print(f"  lsq tiny {C}/{P}/{N}: status {res.status} nfev {res.nfev} cost {res.cost:.6f}")
    # unobserved camera and point (zero Jacobian columns), single-observation points
    pb = drop_observations(make_problem(5, 40, 200, seed=9), cameras=(3,), points=(7,))
    S = ba.create_sparsity_matrix(5, 40, pb.n_obs, pb.camera_indices, pb.point_indices)
    res = least_squares(ba.compute_residuals, pb.x0, jac_sparsity=S, verbose=0, x_scale="jac",
                        ftol=1e-10, method="trf", args=pb.args)
    out["gaps_x0"], out["gaps_x"], out["gaps_fun"] = pb.x0, res.x, res.fun
    out["gaps_summary"] = np.array([res.status, res.nfev, res.njev, res.cost,
                                    np.sqrt(np.mean(res.fun ** 2)), res.optimality])
    print(f"  lsq gaps 5/40/{pb.n_obs}: status {res.status} nfev {res.nfev} cost {res.cost:.6f}")
    # cameras on a ring looking inward: rotation vectors up to pi inside a full solve
    pb = make_ring_problem(12, 150, 900, seed=1)
    S = ba.create_sparsity_matrix(12, 150, 900, pb.camera_indices, pb.point_indices)
    res = least_squares(ba.compute_residuals, pb.x0, jac_sparsity=S, verbose=0, x_scale="jac",
                        ftol=1e-10, method="trf", args=pb.args)
    out["ring_x0"], out["ring_x"], out["ring_fun"] = pb.x0, res.x, res.fun
    out["ring_summary"] = np.array([res.status, res.nfev, res.njev, res.cost,
                                    np.sqrt(np.mean(res.fun ** 2)), res.optimality])
    print(f"  lsq ring 12/150/900: status {res.status} nfev {res.nfev} cost {res.cost:.6f}")
    out["n_cases"] = np.array(3)
    return out


def pack_cases():
    """A4: rotation log/exp per camera as scipy does it at sfm.py:255,277."""
    rng = np.random.default_rng(7)
    w = rng.normal(0, 1.0, (12, 3))
    w[0] = 0.0
    w[1] *= 1e-9
    w[2] = w[2] / np.linalg.norm(w[2]) * (np.pi - 1e-6)     # near pi
    w[3] = w[3] / np.linalg.norm(w[3]) * 3.0
    R = Rot.from_rotvec(w).as_matrix()
    back = Rot.from_matrix(R).as_rotvec()
    T = rng.normal(0, 2.0, (12, 3))
    H = np.tile(np.eye(4), (12, 1, 1))
    H[:, :3, :3] = R
    H[:, :3, 3] = T
    return {"w": w, "R": R, "rotvec_from_matrix": back, "H": H}


def lsq_cfg2(ba):
    """The SceauxCastle-scale synthetic (11/3000/10000): full scipy run, ~6-7 min single thread."""
    pb = make_problem(11, 3000, 10000, seed=0)
    t = time.time()
    S = ba.create_sparsity_matrix(11, 3000, 10000, pb.camera_indices, pb.point_indices)
    t_sp = time.time() - t
    buf = io.StringIO()
    t = time.time()
    with redirect_stdout(buf):
        res = least_squares(ba.compute_residuals, pb.x0, jac_sparsity=S, verbose=2, x_scale="jac",
                            ftol=1e-10, method="trf", args=pb.args)
    t_lsq = time.time() - t
    rows = []
    for line in buf.getvalue().splitlines():
        m = re.match(r"\s*(\d+)\s+(\d+)\s+([0-9.e+-]+)\s*([0-9.e+-]+)?\s*([0-9.e+-]+)?\s*([0-9.e+-]+)?", line)
        if m:
            rows.append([float(v) if v else None for v in m.groups()])
    summary = dict(
        config=dict(n_cameras=11, n_points=3000, n_obs=10000, seed=0, ftol=1e-10),
        scipy_version=__import__("scipy").__version__, numpy_version=np.__version__,
        status=int(res.status), nfev=int(res.nfev), njev=int(res.njev), cost=float(res.cost),
        rmse=float(np.sqrt(np.mean(res.fun ** 2))), optimality=float(res.optimality),
        rmse0=float(np.sqrt(np.mean(ba.compute_residuals(pb.x0, *pb.args) ** 2))),
        seconds_least_squares=t_lsq, seconds_create_sparsity=t_sp,
        iterations_per_sec=res.njev / t_lsq, host="build container, 1 thread",
        table_columns=["iteration", "nfev", "cost", "cost_reduction", "step_norm", "optimality"],
        table=rows)
    with open(os.path.join(OUT, "scipy_cfg2_run.json"), "w") as f:
        json.dump(summary, f, indent=1)
    np.savez_compressed(os.path.join(OUT, "scipy_cfg2_x.npz"), x=res.x, fun=res.fun)
    print(f"  cfg2: {res.njev} iterations in {t_lsq:.1f}s, rmse {summary['rmse']:.9f}")


def oracle_full(name):
    """Recorded run of the ORACLE (not the reference: scipy's own path would need ~20 min per iteration at cfg4,
    SURVEY.md section 6) with the settings the HIP path ships -- PCG on the implicit Schur complement, Schur-diagonal
    block preconditioner, adaptive forcing term 1e-2 ... 1e-1 -- on a BASELINE.json configuration at full size.
    What the GPU tests compare at sizes the oracle cannot be run at inside the suite: status, nfev, njev, cost,
    RMSE and the PCG iterations of every outer iteration."""
    sys.path.insert(0, ROOT)
    from sfmba.synthetic import make_config
    pb = make_config(name)
    rec, o, dt = _oracle_record(pb, name)
    with open(os.path.join(OUT, f"oracle_{name}.json"), "w") as f:
        json.dump(rec, f, indent=1)
    print(f"  oracle {name}: status {o.status} nfev {o.nfev} cost {o.cost!r} pcg {rec['pcg_iterations']} in {dt:.0f}s")


def _oracle_record(pb, name):
    """oracle.trf_schur on `pb` with the shipped settings -> (the record oracle_<name>.json holds, result, seconds)."""
    from oracle import ba_oracle as orc
    from sfmba.synthetic import CONFIGS
    t = time.time()
    o = orc.trf_schur(pb.x0, *pb.args, ftol=1e-10, linear="pcg", pcg_tol=1e-2, pcg_tol_max=0.1, precond="schur",
                      verbose=1)
    dt = time.time() - t
    rec = dict(config=dict(name=name, n_cameras=CONFIGS[name][0], n_points=CONFIGS[name][1], n_obs=CONFIGS[name][2],
                           seed=0, ftol=1e-10),
               oracle_settings=dict(linear="pcg", pcg_tol=1e-2, pcg_tol_max=0.1, precond="schur", reg_min=1e-6),
               numpy_version=np.__version__, seconds=dt,
               status=int(o.status), nfev=int(o.nfev), njev=int(o.njev), cost=float(o.cost),
               rmse=float(np.sqrt(np.mean(o.fun ** 2))), optimality=float(o.optimality),
               cost0=float(o.history[0]["cost"]),
               pcg_iterations=[int(h["pcg_iters"]) for h in o.history[1:]],
               cost_per_iteration=[float(h["cost"]) for h in o.history],
               x_checksum=dict(sum=float(np.sum(o.x)), abs_sum=float(np.sum(np.abs(o.x))),
                               cams_sum=float(np.sum(o.x[:6 * pb.n_cameras]))))
    return rec, o, dt


def oracle_shard(name, world):
    """The same recorded run for RANK 0'S SHARE of a `world`-way observation sharding of a BASELINE.json configuration
    (sfmba.dist.partition_points / shard_problem: all cameras, the rank's own points and observations, solved as a
    problem of its own) -- what a handle that runs the sharded forms with a world of one must reproduce.  On top of
    oracle_full's fields: the shard's own sizes, and per outer iteration the two ratios the oracle's termination test
    compares with 1 (ba_oracle.trf_schur, check_termination): actual_reduction / (ftol * cost before the step) and
    step_norm / (xtol * (xtol + |x|)).  A count-for-count comparison with another implementation is only fair where
    none of them is near 1; tests/test_oracle_golden.py asserts that from the file."""
    sys.path.insert(0, ROOT)
    from sfmba.dist import partition_points, shard_problem
    from sfmba.synthetic import make_config
    pb = make_config(name)
    pb = shard_problem(pb, partition_points(pb.point_indices, pb.n_points, world)[0])
    rec, o, dt = _oracle_record(pb, name)
    ftol, xtol = rec["config"]["ftol"], 1e-8                       # (xtol: trf_schur's default, as in oracle_full)
    h = o.history
    rec["shard"] = dict(rank=0, world=world, n_points=int(pb.n_points), n_obs=int(pb.n_obs))
    rec["xtol"] = xtol
    rec["ftol_ratio_per_iteration"] = [float(h[k]["reduction"] / (ftol * h[k - 1]["cost"])) for k in range(1, len(h))]
    rec["xtol_ratio_per_iteration"] = [float(h[k]["step_norm"] / (xtol * (xtol + h[k]["x_norm"]))) for k in range(1, len(h))]
    with open(os.path.join(OUT, f"oracle_{name}_shard{world}.json"), "w") as f:
        json.dump(rec, f, indent=1)
    print(f"  oracle {name} shard 0 of {world} ({pb.n_cameras} / {pb.n_points} / {pb.n_obs}): status {o.status} nfev {o.nfev} "
          f"cost {o.cost!r} pcg {rec['pcg_iterations']} in {dt:.0f}s\n    ftol ratios {rec['ftol_ratio_per_iteration']}\n"
          f"    xtol ratios {rec['xtol_ratio_per_iteration']}")


def lsq_growing(ba):
    """scipy.optimize.least_squares with the kwargs of sfm.py:266-268 driving the REFERENCE's compute_residuals on
    every stage of a growing reconstruction cut from the SceauxCastle-scale synthetic (sfm.py:59-71: BA after every
    registration, each call warm-started from the previous result).  Pack / unpack as sfm.py:248-262, 271-281 with
    scipy's Rotation.  Stage inputs are derived from ``sfmba.synthetic.growing_reconstruction`` (structure) and
    scipy's own previous result (state), so a test can replay the chain with its own solver."""
    from sfmba.synthetic import growing_reconstruction
    pb = make_problem(11, 3000, 10000, seed=0)
    order = [0, 5, 2, 7, 1, 6, 3, 4, 10, 8, 9]
    C = pb.n_cameras
    cams0 = pb.x0[:6 * C].reshape(C, 6)
    pts0 = pb.x0[6 * C:].reshape(-1, 3)
    H = [np.eye(4) for _ in range(C)]
    X3d = np.zeros((0, 3))
    stages = []
    arrays = {"order": np.array(order)}
    for k, st in enumerate(growing_reconstruction(pb, order)):
        for c in st["new_camera"]:                                   # "PnP": the noisy initial pose of the generator
            H[c][:3, :3] = Rot.from_rotvec(cams0[c, :3]).as_matrix()
            H[c][:3, 3] = cams0[c, 3:]
        new = st["cloud"][len(X3d):]
        X3d = np.vstack([X3d, pts0[new]])                            # "triangulation": the noisy initial points
        data = st["observations"]
        pt_indices, cam_indices, pt2ds = map(np.array, zip(*[(p, c, uv) for p, c, uv in data]))
        reg = [c for c in range(C) if st["registered"][c]]
        camera_map = {c: i for i, c in enumerate(reg)}
        params = [(Rot.from_matrix(H[c][:3, :3]).as_rotvec(), H[c][:3, 3].flatten()) for c in reg]
        camera_indices = np.array([camera_map[c] for c in cam_indices])
        x0 = np.hstack([np.hstack([e, t]).ravel() for e, t in params] + [X3d.ravel()])
        n_cam, n_points, n_obs = len(reg), len(X3d), len(pt_indices)
        S = ba.create_sparsity_matrix(n_cam, n_points, n_obs, camera_indices, pt_indices)
        t = time.time()
        res = least_squares(ba.compute_residuals, x0, jac_sparsity=S, verbose=0, x_scale="jac", ftol=1e-10,
                            method="trf", args=(n_cam, n_points, camera_indices, pt_indices, pt2ds, pb.K))
        dt = time.time() - t
        r0 = ba.compute_residuals(x0, n_cam, n_points, camera_indices, pt_indices, pt2ds, pb.K)
        stages.append(dict(stage=k, n_cameras=n_cam, n_points=n_points, n_obs=n_obs, status=int(res.status),
                           nfev=int(res.nfev), njev=int(res.njev), cost=float(res.cost),
                           rmse=float(np.sqrt(np.mean(res.fun ** 2))), rmse0=float(np.sqrt(np.mean(r0 ** 2))),
                           optimality=float(res.optimality), seconds=dt))
        arrays[f"s{k:02d}_x0"] = x0          # (stage inputs: a test can replay every stage from scipy's own start)
        print(f"  growing stage {k}: {n_cam}/{n_points}/{n_obs} status {res.status} njev {res.njev} "
              f"rmse {stages[-1]['rmse0']:.6f} -> {stages[-1]['rmse']:.9f} in {dt:.0f}s", flush=True)
        cp = res.x[:n_cam * 6].reshape((n_cam, 6))
        for c, n in camera_map.items():
            H[c] = np.eye(4)
            H[c][:3, :3] = Rot.from_rotvec(cp[n, :3]).as_matrix()
            H[c][:3, 3] = cp[n, 3:]
        X3d = res.x[n_cam * 6:].reshape((n_points, 3))
    rec = dict(base=dict(n_cameras=11, n_points=3000, n_obs=10000, seed=0), order=order, ftol=1e-10,
               scipy_version=__import__("scipy").__version__, numpy_version=np.__version__,
               host="build container, 1 thread", stages=stages)
    with open(os.path.join(OUT, "scipy_growing_run.json"), "w") as f:
        json.dump(rec, f, indent=1)
    np.savez_compressed(os.path.join(OUT, "scipy_growing_x.npz"), **arrays)


# settings of the two forms of the Schur PCG the HIP path ships (tests/test_gpu_parity.py::_oracle_kwargs)
DENSE_KW = dict(linear="pcg", pcg_tol=1e-3, precond="schur_exact")
IMPLICIT_KW = dict(linear="pcg", pcg_tol=1e-2, pcg_tol_max=0.1, precond="schur")


def lsq_fixed(ba):
    """create_sparsity_matrix(..., fixed_camera_indices) handed to scipy (REF bundle_adjustment.py:6,13-14): the held
    cameras' columns stay zero in scipy's finite-difference Jacobian, so their parameters do not move.  One camera held
    (the gauge keeps 1 dof: scale) and two (gauge fully pinned).  The held cameras start at their true poses (somebody who
    holds a camera still trusts it).
    What the capture shows: scipy holds them still (they move by <= 1e-13) but does NOT reach the minimum of the
    remaining parameters -- its column grouping (_numdiff.py:216-274) puts a held camera's structurally empty columns
    into a group with point columns that share rows with it, the forward difference then perturbs the held parameter
    too (_numdiff.py:671-676) and books the change under the point columns: the Jacobian is wrong there, the ratio test
    shrinks the radius step after step and xtol ends the run at a cost above the minimum.  The fixture therefore pins
    "held cameras do not move" and "cost not above scipy's", not RMSE equality."""
    out = {}
    for k, (C, P, N, seed, fixed) in enumerate([(4, 30, 120, 11, (0,)), (6, 60, 400, 12, (0, 2)), (6, 60, 400, 12, (5,))]):
        pb = make_problem(C, P, N, seed=seed)
        x0 = pb.x0.copy()
        for c in fixed:
            x0[6 * c:6 * c + 6] = pb.x_true[6 * c:6 * c + 6]
        S = ba.create_sparsity_matrix(C, P, N, pb.camera_indices, pb.point_indices, fixed_camera_indices=fixed)
        res = least_squares(ba.compute_residuals, x0, jac_sparsity=S, verbose=0, x_scale="jac",
                            ftol=1e-10, method="trf", args=pb.args)
        pre = f"f{k}_"
        out[pre + "dims"] = np.array([C, P, N])
        out[pre + "seed"] = np.array(seed)
        out[pre + "fixed"] = np.array(fixed, dtype=np.int64)
        out[pre + "x0"], out[pre + "x"], out[pre + "fun"] = x0, res.x, res.fun
        out[pre + "summary"] = np.array([res.status, res.nfev, res.njev, res.cost, np.sqrt(np.mean(res.fun ** 2)),
                                         res.optimality])
        moved = np.abs(res.x[:6 * C].reshape(C, 6) - x0[:6 * C].reshape(C, 6)).max(axis=1)
        print(f"  lsq fixed {fixed} {C}/{P}/{N}: status {res.status} nfev {res.nfev} cost {res.cost:.6f} "
              f"held cameras moved by {moved[list(fixed)].max():.1e}, free ones by >= {np.delete(moved, list(fixed)).min():.1e}")
    out["n_cases"] = np.array(3)
    return out


def param_bounds(ba):
    """"gauge-aligned parameters (tolerance measured and stated)".  For every scipy result the
    fixtures hold -- the five tiny runs, the SceauxCastle-scale run, the ten stages of the growing reconstruction --
    the ORACLE is run from the same start with the settings the HIP path ships, its parameter vector is mapped onto
    scipy's by the best 7-dof similarity (oracle.similarity_align, fitted on the points at least two cameras see: a
    point seen once has no defined depth) and the distances are recorded: what the GPU tests then allow the HIP path,
    times two.  (The fixed-camera captures are not in this table: scipy does not reach the minimum there, see
    lsq_fixed.)  Also stores scipy's final x of every growing stage (stages 0..8: read back from the next stage's
    start, which is that result written through sfm.py:271-281; the last stage: scipy re-run from its recorded start)."""
    sys.path.insert(0, ROOT)
    from oracle import ba_oracle as orc
    from sfmba.synthetic import growing_reconstruction

    def measure(tag, x_scipy, fun_scipy, x0, args, kw):
        C, P, ci, pi = args[0], args[1], np.asarray(args[2]), np.asarray(args[3])
        o = orc.trf_schur(x0, *args, ftol=1e-10, **kw)
        mv = orc.multi_view_points(C, P, ci, pi)
        xa, (s, _, _) = orc.similarity_align(o.x, x_scipy, C, P, fit_points=mv)
        seen = np.bincount(ci, minlength=C) > 0
        d = orc.parameter_distance(xa, x_scipy, C, P, observed_cameras=seen, points=mv)
        raw = orc.parameter_distance(o.x, x_scipy, C, P, observed_cameras=seen, points=mv)
        d.update(case=tag, settings="dense" if kw is DENSE_KW else "implicit", points_compared=int(mv.sum()), n_points=int(P),
                 fun_max=float(np.abs(o.fun - fun_scipy).max()), scale=s,
                 rmse_oracle=float(np.sqrt(np.mean(o.fun ** 2))), rmse_scipy=float(np.sqrt(np.mean(fun_scipy ** 2))),
                 unaligned_points_rms=raw["points_rms"])
        print(f"  {tag:28s} {d['settings']:8s} points rms {d['points_rms']:.2e} max {d['points_max']:.2e} centres {d['centres_max']:.2e} "
              f"rot {d['rot_deg_max']:.2e} deg  fun {d['fun_max']:.2e}  ({d['points_compared']} of {P} points; unaligned rms "
              f"{raw['points_rms']:.2e})", flush=True)
        return d

    rows = []
    g = np.load(os.path.join(OUT, "lsq_tiny_cases.npz"))
    for k in range(int(g["n_cases"])):
        pre = f"l{k}_"
        C, P, N = (int(v) for v in g[pre + "dims"])
        pb = make_problem(C, P, N, seed=int(g[pre + "seed"]))
        for kw in (DENSE_KW, IMPLICIT_KW):
            rows.append(measure(f"tiny{k}_{C}_{P}_{N}", g[pre + "x"], g[pre + "fun"], pb.x0, pb.args, kw))
    pb = drop_observations(make_problem(5, 40, 200, seed=9), cameras=(3,), points=(7,))
    for kw in (DENSE_KW, IMPLICIT_KW):
        rows.append(measure("gaps_5_40", g["gaps_x"], g["gaps_fun"], pb.x0, pb.args, kw))
    pb = make_ring_problem(12, 150, 900, seed=1)
    for kw in (DENSE_KW, IMPLICIT_KW):
        rows.append(measure("ring_12_150_900", g["ring_x"], g["ring_fun"], pb.x0, pb.args, kw))
    g2 = np.load(os.path.join(OUT, "scipy_cfg2_x.npz"))
    pb = make_problem(11, 3000, 10000, seed=0)
    for kw in (DENSE_KW, IMPLICIT_KW):
        rows.append(measure("cfg2_11_3000_10000", g2["x"], g2["fun"], pb.x0, pb.args, kw))

    # growing reconstruction: scipy's final x per stage
    rec = json.load(open(os.path.join(OUT, "scipy_growing_run.json")))
    arrs = np.load(os.path.join(OUT, "scipy_growing_x.npz"))
    stages = list(growing_reconstruction(pb, rec["order"]))
    finals = {}
    stage_args = []
    for k, st in enumerate(stages):
        reg = [c for c in range(pb.n_cameras) if st["registered"][c]]
        cmap = {c: i for i, c in enumerate(reg)}
        pt_indices, cam_ids, pt2ds = map(np.array, zip(*[(p, c, uv) for p, c, uv in st["observations"]]))
        stage_args.append((len(reg), len(st["cloud"]), np.array([cmap[c] for c in cam_ids]), pt_indices, pt2ds, pb.K))
    for k in range(len(stages) - 1):
        reg_k = [c for c in range(pb.n_cameras) if stages[k]["registered"][c]]
        reg_n = [c for c in range(pb.n_cameras) if stages[k + 1]["registered"][c]]
        xn = arrs[f"s{k + 1:02d}_x0"]
        cams_n = xn[:6 * len(reg_n)].reshape(len(reg_n), 6)
        n_pts = len(stages[k]["cloud"])
        finals[k] = np.concatenate([np.concatenate([cams_n[reg_n.index(c)] for c in reg_k]),
                                    xn[6 * len(reg_n):6 * len(reg_n) + 3 * n_pts]])
    k = len(stages) - 1
    a = stage_args[k]
    have = os.path.join(OUT, "scipy_growing_xfinal.npz")
    if os.path.exists(have) and f"s{k:02d}_x" in np.load(have):          # (the 3.5-minute scipy run is done once)
        finals[k] = np.load(have)[f"s{k:02d}_x"]
    else:
        S = ba.create_sparsity_matrix(a[0], a[1], len(a[2]), a[2], a[3])
        t = time.time()
        res = least_squares(ba.compute_residuals, arrs[f"s{k:02d}_x0"], jac_sparsity=S, verbose=0, x_scale="jac", ftol=1e-10,
                            method="trf", args=a)
        assert abs(float(np.sqrt(np.mean(res.fun ** 2))) - rec["stages"][k]["rmse"]) < 1e-12, "last stage does not reproduce the record"
        print(f"  last growing stage re-run with scipy in {time.time() - t:.0f}s: rmse {np.sqrt(np.mean(res.fun ** 2)):.12f} == record")
        finals[k] = res.x
    np.savez_compressed(have, **{f"s{k:02d}_x": v for k, v in finals.items()})
    for k in range(len(stages)):
        a = stage_args[k]
        fs = ba.compute_residuals(finals[k], *a)
        assert abs(float(np.sqrt(np.mean(fs ** 2))) - rec["stages"][k]["rmse"]) < 1e-9, (k, "derived final x does not give the recorded rmse")
        rows.append(measure(f"growing_stage{k}", finals[k], fs, arrs[f"s{k:02d}_x0"], a, DENSE_KW))
    with open(os.path.join(OUT, "param_bounds.json"), "w") as f:
        json.dump(dict(note="distance between the ORACLE's and scipy's final parameters after the best 7-dof similarity "
                            "(fitted on the points); scipy stops on ftol in a slow tail, the Schur step converges further",
                       scipy_version=__import__("scipy").__version__, rows=rows), f, indent=1)


REF_TRI = "/root/reference/cv2_lite/triangulate_points.py"
TRI_BOUND_FACTOR = 100.0       # fused multiply-adds, the Jacobi rotation order and summation order of the kernel


def triangulate_cases():
    """tests/golden/triangulate_cases.npz: K_SCEAUX, two synthetic camera matrices, 100 noisy pixel pairs and the output
    of the reference's `triangulate_points_linear2` on them; tests/golden/triangulate_bounds.json: the distance of the
    numpy restatement (tests/triangulate_ref.py) to the reference on that set, and to the SVD of the same rows on the
    tracks of the GPU tests' problem, each with the bound (x TRI_BOUND_FACTOR) the kernel is held to.  Data only."""
    spec = importlib.util.spec_from_file_location("ref_tri", REF_TRI)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import triangulate_ref as tr
    from sfmba.synthetic import K_SCEAUX

    rng = np.random.default_rng(2024)
    n = 100
    cams = np.array([[0.03, -0.12, 0.02, -0.6, 0.1, 0.2], [-0.05, 0.15, -0.04, 0.7, -0.2, -0.1]])
    M = tr.projection_matrices(cams.ravel(), 2, K_SCEAUX)
    X = rng.normal(0.0, 1.0, (n, 3)) + np.array([0.0, 0.0, 10.0])
    Xh = np.hstack([X, np.ones((n, 1))])
    pts = []
    for k in range(2):
        p = Xh @ M[k].T
        pts.append((p[:, :2] / p[:, 2:3] + rng.normal(0.0, 0.5, (n, 2))).T.copy())
    X_ref = ref.triangulate_points_linear2(M[0], M[1], pts[0], pts[1])
    np.savez_compressed(os.path.join(OUT, "triangulate_cases.npz"), K=K_SCEAUX, M1=M[0], M2=M[1], pts1=pts[0],
                        pts2=pts[1], X_ref=X_ref)

    # the restatement on the fixture, through the same K^-1 M -> (rotation vector, centre) route the library takes
    c2 = np.concatenate([tr.cameras_from_projection(M[0], K_SCEAUX), tr.cameras_from_projection(M[1], K_SCEAUX)])
    uv = np.stack([pts[0].T, pts[1].T], axis=1).reshape(2 * n, 2)
    args = (2, n, np.tile([0, 1], n), np.repeat(np.arange(n), 2), uv, K_SCEAUX)
    lin = tr.triangulate(np.concatenate([c2, np.zeros(3 * n)]), args, max_iter=0, min_angle_deg=-np.inf,
                         min_depth=-np.inf)["linear"]
    d_fix = float(np.abs(lin - X_ref[:3].T).max())

    # ... and on the tracks of the GPU tests' problem against the SVD of the same rows
    pb = make_problem(6, 300, 1500, seed=3)
    C, P, ci, pi, uv, K = pb.args
    full = tr.triangulate(pb.x_true, pb.args, max_iter=0)
    Mc = tr.projection_matrices(pb.x_true, C, K)
    order, ptr = tr.stored_runs(pi, P)
    cams = pb.x_true[:6 * C].reshape(C, 6)
    d_pb, n_cmp, n_two = 0.0, 0, 0
    for p in range(P):
        idx = order[ptr[p]:ptr[p + 1]]
        if len(idx) < 2:
            continue
        n_two += 1
        Xs = tr.svd_point(tr.dlt_rows(Mc[ci[idx]], uv[idx]))
        if tr.widest_angle_deg(Xs, cams[ci[idx], 3:]) < 2.0:
            continue
        n_cmp += 1
        d_pb = max(d_pb, float(np.abs(full["linear"][p] - Xs).max() / max(1.0, np.abs(Xs).max())))
    rec = dict(factor=TRI_BOUND_FACTOR,
               fixture=dict(measured_abs=d_fix, bound_abs=TRI_BOUND_FACTOR * d_fix),
               problem=dict(spec=[6, 300, 1500, 3], tracks_two_views=n_two, tracks_compared=n_cmp,
                            measured_rel=d_pb, bound_rel=TRI_BOUND_FACTOR * d_pb))
    with open(os.path.join(OUT, "triangulate_bounds.json"), "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg2", action="store_true")
    ap.add_argument("--full", choices=("cfg3", "cfg4", "cfg5"))
    ap.add_argument("--shard", nargs=2, metavar=("NAME", "G"), help="oracle run of rank 0's share of a G-way sharding")
    ap.add_argument("--growing", action="store_true")
    ap.add_argument("--fixed", action="store_true")
    ap.add_argument("--params", action="store_true")
    ap.add_argument("--triangulate", action="store_true")
    a = ap.parse_args()
    if a.triangulate:
        triangulate_cases()
        return
    if a.full:                                   # oracle only: needs no reference
        os.makedirs(OUT, exist_ok=True)
        oracle_full(a.full)
        return
    if a.shard:
        if a.shard[0] not in ("cfg3", "cfg4", "cfg5"):
            ap.error("--shard NAME: one of cfg3, cfg4, cfg5")
        os.makedirs(OUT, exist_ok=True)
        oracle_shard(a.shard[0], int(a.shard[1]))
        return
    if a.growing:
        lsq_growing(load_ref())
        return
    if a.fixed:
        np.savez_compressed(os.path.join(OUT, "lsq_fixed_cases.npz"), **lsq_fixed(load_ref()))
        return
    if a.params:
        param_bounds(load_ref())
        return
    if not os.path.exists(REF_BA):
        sys.exit("reference not present: fixtures can only be generated in the build container")
    os.makedirs(OUT, exist_ok=True)
    ba = load_ref()
    np.savez_compressed(os.path.join(OUT, "residual_cases.npz"), **residual_cases(ba))
    np.savez_compressed(os.path.join(OUT, "sparsity_cases.npz"), **sparsity_cases(ba))
    np.savez_compressed(os.path.join(OUT, "jacobian_fd_cases.npz"), **jacobian_cases(ba))
    np.savez_compressed(os.path.join(OUT, "lsq_tiny_cases.npz"), **lsq_tiny(ba))
    np.savez_compressed(os.path.join(OUT, "pack_cases.npz"), **pack_cases())
    print("fast fixtures written to", OUT)
    if a.cfg2:
        lsq_cfg2(ba)


if __name__ == "__main__":
    main()
