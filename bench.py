#!/usr/bin/env python3
"""bench.py -- BA iterations/sec of the MI355X bundle-adjustment path (BASELINE.json metric).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--workload cfg4] [--dump-outputs DIR]
    python bench.py --full [--no-cpu-baseline] [--no-per-call] ...
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

A plain run sets up, warms up, times the K steps and prints the line.  `--full` adds what takes runs of its own: the
first solve on a fresh handle, the J-free companion, the residual+Jacobian kernel without its point sums, per-call
least_squares() timings and the scipy CPU baseline.  `--dump-outputs DIR` writes what the last timed solve returned
(x, its residual vector and gradient, cost, rmse, optimality) as DIR/<name>.npy.

A *step* is one outer (trust-region) iteration of the solver that replaces the reference's
``least_squares`` call (/root/reference/sfm_lite/sfm.py:266-268): Jacobian sweep, normal-equation
blocks, Schur-complement PCG, trial residual sweep, accept/reject.  The K timed steps are produced by
back-to-back solves from the same x0 with the reference's own tolerance (ftol=1e-10), the last solve
capped so that exactly K iterations fall in the timed region.  Problem arrays are resident in HBM
before the clock starts; only x0 (6C+3P doubles) crosses PCIe per solve.

N = 1: the 1000-camera / 100k-point / 1M-observation synthetic (BASELINE.json: the problem the >=100x
target is quoted on).  N > 1, default `--scaling strong` (BASELINE.json configs[3], north_star ">= 6x at 8 GPUs"):
the SAME 1M-observation problem, observations cut at point boundaries into N shards (sfmba.dist.partition_points
/ shard_problem), cameras replicated, camera-side normal-equation blocks, reduced right-hand side and PCG
products all-reduced; `value` = outer iterations of the whole problem per second, comparable with the N = 1
number.  `--scaling weak`: every rank owns its own cfg-sized shard that shares the cameras; `value` then counts
shard-iterations summed over ranks (a different unit, labelled as such).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, os.path.join(ROOT, "sfm-python_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

HBM_PEAK_GBS = 8000.0          # MI355X HBM3E spec peak (/opt/skills/guides/MI355X_MICROARCH.md)
DUMP_BYTES = 64 << 20          # --dump-outputs writes at most this much in all
DUMP_ELEMS = 1 << 21           # ... and at most this many entries per array


def dump_outputs(out_dir, arrays):
    """Write every array as <out_dir>/<name>.npy in float64.  An array of more than DUMP_ELEMS entries is written as the
    entries at a fixed, seeded sample of its indices (numpy default_rng(0), sorted): the same for every run of the same
    arguments, so two builds compare entry for entry."""
    os.makedirs(out_dir, exist_ok=True)
    total = 0
    for name, v in arrays.items():
        v = np.ascontiguousarray(v, dtype=np.float64).ravel()
        if v.size > DUMP_ELEMS:
            print(f"[bench] {name}: {v.size} entries, writing a seeded sample of {DUMP_ELEMS}", file=sys.stderr, flush=True)
            v = v[np.sort(np.random.default_rng(0).choice(v.size, DUMP_ELEMS, replace=False))]
        total += v.nbytes
        if total > DUMP_BYTES:
            raise RuntimeError(f"--dump-outputs: more than {DUMP_BYTES} bytes")
        np.save(os.path.join(out_dir, name + ".npy"), v)


def k1_bytes_f32(C, P, N):
    """fp32-storage mode: idx 8 + uv 8 read, r 8 + Jacobian 48 written per observation; point rows as k1_bytes."""
    return 72 * N + 96 * P + 48 * C


def k1_bytes(C, P, N):
    """Algorithmic bytes of one residual+Jacobian launch: per observation read
    cam_idx 4 + pt_idx 4 + uv 16, write r 16 + d r/d w 48 + d r/d X 48 = 136 B; once per point 24 B, per
    camera 48 B.  The launch also leaves the point half of the normal equations, V_p (48 B) and g_p
    (24 B) per point, summed from the blocks it holds in registers: 96 B per point in all.  SURVEY.md section 8d
    counts 184 B per observation because it also writes d r/d T, which is -d r/d X and is not stored (see
    k1_bytes_survey for that accounting)."""
    return 136 * N + 96 * P + 48 * C


def k1_bytes_survey(C, P, N):
    return 184 * N + 96 * P + 48 * C


def cpu_baseline(workload_dims, seconds_budget=25.0):
    """scipy.optimize.least_squares with the reference's kwargs driving the oracle's per-observation
    restatement of compute_residuals (baseline B1) on a bounded sample of the same
    workload, scaled linearly in n_obs.  One Python thread (the loop is pure Python)."""
    from scipy.optimize import least_squares
    import sfmba
    from oracle import ba_oracle as orc
    C, P, N = workload_dims
    # sample: same cameras, same mean track length, n_obs chosen for ~seconds_budget of CPU work:
    # cost ~ 15.7 us/obs/eval x (2 Jacobians x ~30 colour groups + 2) evals
    us_per_obs = 16e-6
    n_s = int(max(2000, min(N, seconds_budget / (us_per_obs * 62))))
    p_s = max(C // 4, int(round(n_s * P / N)))
    pb = sfmba.make_problem(C, p_s, n_s, seed=1)
    S = sfmba.create_sparsity_matrix(C, p_s, n_s, pb.camera_indices, pb.point_indices)
    out = {}
    for kind, fun in (("loop", orc.compute_residuals_loop), ("vectorized", orc.compute_residuals)):
        t = time.time()
        res = least_squares(fun, pb.x0, jac_sparsity=S, verbose=0, x_scale="jac", ftol=1e-10,
                            method="trf", max_nfev=2, args=pb.args)
        dt = time.time() - t
        out[kind] = dict(seconds=dt, njev=int(res.njev), nfev=int(res.nfev),
                         it_per_s_sample=res.njev / dt, it_per_s_scaled=res.njev / dt * n_s / N)
    sample = (f"scipy least_squares(method='trf', x_scale='jac', jac_sparsity, max_nfev=2) on a "
              f"{C}-camera/{p_s}-point/{n_s}-observation sample of the workload, njev/time scaled by "
              f"n_obs ratio {n_s}/{N}; per-observation Python residual (oracle port of "
              f"bundle_adjustment.py:20-42); {out['loop']['seconds']:.1f} s of CPU work")
    return dict(value=out["loop"]["it_per_s_scaled"], unit="iterations/s", cores=1, kind="port",
                sample=sample, host_cores=os.cpu_count(),
                vectorized_numpy_value=out["vectorized"]["it_per_s_scaled"],
                detail=out)


def per_call_times(workload, storage_bits):
    """What a user of the drop-in sees: wall time of ONE sfmba.least_squares(...) call with the reference's
    kwargs (sfm.py:266-268) -- argument conversion, set_problem (conversion, structure tables, upload), solve,
    download of x; like the reference (sfm.py:271,281) the caller reads result.x and drops the result, so fun and
    grad are never downloaded -- for the bench workload and for the SceauxCastle-scale problem the reference itself
    produces.  The reference calls BA once per fused edge on a growing problem (sfm.py:59-71), so three warm cases
    are timed besides the cold first call of a handle: `rebuilt` -- the previous problem of the handle differs from
    the first observation on (everything is converted and uploaded again); `grown` -- the previous problem was the
    first 99 % of the points of this one (an edge that only triangulates new points: the prefix is re-used, the tail
    uploaded); `same` -- identical arrays (e.g. a second BA pass)."""
    import sfmba
    out = {}
    for name in dict.fromkeys([workload, "cfg2"]):
        pb = sfmba.make_config(name)
        n_head = int(np.searchsorted(pb.point_indices, int(0.99 * pb.n_points), side="left"))
        p_head = int(0.99 * pb.n_points)
        head_args = (pb.n_cameras, p_head, pb.camera_indices[:n_head], pb.point_indices[:n_head], pb.points_2d[:n_head], pb.K)
        head_x0 = pb.x0[:6 * pb.n_cameras + 3 * p_head]
        other_uv = pb.points_2d.copy()
        other_uv[0, 0] += 1                                   # differs from the first observation on
        other_args = pb.args[:4] + (other_uv, pb.K)
        be = sfmba.Backend(0)

        def call(x0, args):
            t = time.perf_counter()
            res = sfmba.least_squares(sfmba.compute_residuals, x0, jac_sparsity=None, verbose=0, x_scale="jac",
                                      ftol=1e-10, method="trf", args=args, storage_bits=storage_bits, backend=be)
            assert res.x.shape == x0.shape                          # what the reference reads
            return 1e3 * (time.perf_counter() - t), (int(res.iterations), float(res.seconds)), be.problem_reuse()[0]

        cold, info, _ = call(pb.x0, pb.args)
        rebuilt, grown, same, reused_grown = [], [], [], 0
        for k in range(5):
            call(pb.x0, other_args)
            rebuilt.append(call(pb.x0, pb.args)[0])
            call(head_x0, head_args)
            t, info, reused_grown = call(pb.x0, pb.args)
            grown.append(t)
            same.append(call(pb.x0, pb.args)[0])
        med = lambda v: round(sorted(v)[len(v) // 2], 3)      # noqa: E731
        out[name] = {"cold": round(cold, 3), "rebuilt": med(rebuilt), "grown": med(grown), "same": med(same),
                     "observations_reused_when_grown": int(reused_grown), "n_obs": pb.n_obs,
                     "iterations": info[0], "solve_only": round(1e3 * info[1], 3),
                     "iterations_per_s_per_call_rebuilt": round(info[0] / (1e-3 * med(rebuilt)), 1)}
        be.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workload", default="cfg4", choices=["cfg2", "cfg3", "cfg4", "cfg5"])
    ap.add_argument("--shard-of", type=int, default=0, metavar="G",
                    help="N = 1 only: run rank 0's share of the workload sharded G ways (all cameras, 1/G of the points and "
                         "observations) instead of the whole problem -- with --force-exchange the per-rank critical path "
                         "of a G-GPU strong-scaling run, measured on one GPU (DESIGN.md section 9)")
    ap.add_argument("--full", action="store_true",
                    help="also measure what takes runs of its own after the timed steps: first solve on a fresh handle, "
                         "J-free companion, residual+Jacobian kernel without its point sums, per-call timings, CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed solve returned as DIR/<name>.npy (float64, at most 64 MB in all)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the scipy CPU baseline")
    ap.add_argument("--settle", type=float, default=0.5,
                    help="seconds of untimed solves before the warm-up steps (start-up transient of the GPU queue)")
    ap.add_argument("--force-exchange", action="store_true",
                    help="use the collective path even at world size 1 (plumbing check)")
    ap.add_argument("--storage-bits", type=int, default=64, choices=[64, 32],
                    help="64: fp64 streams (configs 2-4); 32: fp32 storage of pixels/residuals/Jacobian with fp64 "
                         "arithmetic and accumulation (config 5)")
    ap.add_argument("--dist-backend", default="nccl", choices=["nccl", "gloo"],
                    help="torch.distributed backend (gloo + --exchange torch + --one-device rehearses N>1 on one GPU)")
    ap.add_argument("--one-device", action="store_true", help="rehearsal: every rank uses cuda:0")
    ap.add_argument("--exchange", default="native", choices=["native", "torch"],
                    help="native: RCCL called from C++ on the solver stream; torch: torch.distributed callback")
    ap.add_argument("--scaling", default="strong", choices=["strong", "weak"],
                    help="N > 1 only.  strong (default): one problem of the workload's size sharded over the ranks; "
                         "weak: one workload-sized shard per rank")
    ap.add_argument("--no-per-call", action="store_true",
                    help="with --full: skip the end-to-end least_squares() call timings")
    ap.add_argument("--no-direct", action="store_true",
                    help="do not map the peers' staging buffers: every collective goes through --exchange "
                         "(default: the direct xGMI all-reduce kernel serves them, --exchange is the fallback)")
    a = ap.parse_args()
    if a.steps < 1:
        raise SystemExit("--steps must be at least 1")

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if a.gpus != world and world > 1:
        raise SystemExit(f"--gpus {a.gpus} but WORLD_SIZE={world}")
    if a.gpus > 1 and world == 1:
        raise SystemExit("launch N>1 with: python -m torch.distributed.run --nproc-per-node N bench.py --gpus N")

    import torch
    import sfmba
    from sfmba import dist as sdist

    if a.one_device:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    C, P, N = sfmba.synthetic.CONFIGS[a.workload]
    stream = torch.cuda.Stream()
    be = sfmba.Backend(local_rank)
    if world > 1 or a.force_exchange:
        import torch.distributed as td
        if world == 1 and "MASTER_ADDR" not in os.environ:
            os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT="29533", RANK="0", WORLD_SIZE="1")
        if a.dist_backend == "nccl":
            td.init_process_group(backend="nccl", device_id=torch.device("cuda", local_rank))
        else:
            td.init_process_group(backend="gloo")
        if world > 1 and a.scaling == "weak":
            pb = sdist.make_sharded_problem(C, P, N, rank, world, seed=0)
        elif world > 1:                    # strong: every rank builds the same problem and keeps its shard of it
            full = sfmba.make_problem(C, P, N, seed=0)
            shard = sdist.partition_points(full.point_indices, full.n_points, world)[rank]
            pb = sdist.shard_problem(full, shard)
            del full
        else:
            pb = sfmba.make_problem(C, P, N, seed=0)
    else:
        td = None
        pb = sfmba.make_problem(C, P, N, seed=0)
    if world == 1 and a.shard_of > 1:
        pb = sdist.shard_problem(pb, sdist.partition_points(pb.point_indices, pb.n_points, a.shard_of)[0])
    scaling = a.scaling if world > 1 else "strong"          # at N = 1 the two coincide
    Cl, Pl, Nl = pb.n_cameras, pb.n_points, pb.n_obs          # this rank's share

    with torch.cuda.stream(stream):
        be.set_stream(stream.cuda_stream)
        be.set_precision(a.storage_bits)
        for kv in os.environ.get("SFMBA_DEBUG", "").split(","):      # A/B of solver forms (tool-level; the library reads no environment)
            if "=" in kv:
                be.debug_option(kv.split("=")[0], int(kv.split("=")[1]))
        be.set_problem(*pb.args)
        ex = None
        if td is not None:
            if a.exchange == "native":
                try:
                    ex = sdist.NativeComm(be, n_obs_local=Nl)
                except Exception as exc:                      # noqa: BLE001 -- e.g. librccl not loadable
                    print(f"[bench] native RCCL transport unavailable ({exc}); using the torch.distributed "
                          f"callback transport", file=sys.stderr, flush=True)
                    a.exchange = "torch"
            if a.exchange == "torch":
                ex = sdist.Exchange(be, n_obs_local=Nl, device="cuda")
            link = None
            link_dropped = False
            if (world > 1 or a.force_exchange) and not a.no_direct:
                try:
                    link = sdist.DirectLink(be, allow_single=a.force_exchange)
                except Exception as exc:                      # noqa: BLE001 -- keep the run alive on the other transport
                    print(f"[bench] direct all-reduce set-up raised ({exc}); continuing without it",
                          file=sys.stderr, flush=True)
                    link = None
                if (link is None or not link.active) and rank == 0:
                    print("[bench] direct all-reduce unavailable (peer mapping or self-test failed); collectives "
                          f"use the {a.exchange} transport", file=sys.stderr, flush=True)

        opt = be.default_options()
        opt.ftol, opt.xtol, opt.gtol = 1e-10, 1e-8, 1e-8           # the reference's ftol, scipy defaults
        opt.profile = 1

        last = {}                  # --dump-outputs: what the last solve of the latest run_iterations() returned

        def run_iterations(k):
            """exactly k outer iterations from back-to-back solves; returns per-solve results"""
            results, left = [], k
            while left > 0:
                opt.max_iter = left
                x, res, _, _ = be.solve(pb.x0, opt, want_fun=False, want_grad=False)
                if a.dump_outputs and res.iterations >= left:
                    last.update(x=x, res=res)
                del x              # no result array is held across the next solve
                if res.iterations <= 0:
                    raise RuntimeError("solver made no progress")
                results.append((int(res.iterations), float(res.rmse), float(res.rmse0), float(res.resjac_avg_us),
                                int(res.resjac_launches), int(res.pcg_iterations), int(res.status),
                                float(res.seconds_total)))
                left -= int(res.iterations)
            return results

        def barrier():
            if td is not None:
                td.barrier()
            torch.cuda.synchronize()

        # prime clocks, code objects and the host launch path (set-up, not steps) with 50 back-to-back
        # launches of the two heaviest non-roofline kernels.  The residual+Jacobian kernel is left out
        # on purpose: its launches in a rocprofv3 trace of this command are then exactly the ones
        # inside solves, the population `roofline.avg_launch_us` averages over.
        primed = {name: be.time_kernel(pb.x0, which, 50) for which, name in
                  ((2, "camera_blocks"), (3, "schur_sweep"))}
        # Settle: on these boxes a process sees one or two ~45 ms stalls of its GPU queue during the first
        # ~100 ms of activity (observed with SFMBA_DEBUG_STALLS=1; none later in 600-solve runs).  Untimed
        # back-to-back solves for half a second keep that start-up transient out of the W + K steps below.
        t_settle = time.perf_counter()
        if td is None:
            while time.perf_counter() - t_settle < a.settle:
                run_iterations(5)
        else:                      # every solve is a sequence of collectives: all ranks must run the same number
            # The first solves of a multi-rank run are also the first time the direct link carries real traffic between
            # THESE devices (the attach self-test covers the collective launches, not the per-camera exchange inside the
            # kernels).  Should a solve fail there on any rank (time-out of a peer: error -5), every rank drops the link
            # and the run continues on the transport registered before it (RCCL / torch.distributed) instead of ending
            # without a line; the line then says so in "transport".
            try:
                run_iterations(5)
                ok = 1
            except sfmba.BackendError as exc:
                ok = 0
                print(f"[bench] rank {rank}: first sharded solve failed ({exc})", file=sys.stderr, flush=True)
            flag = torch.tensor([ok], dtype=torch.int32, device="cuda" if td.get_backend() == "nccl" else "cpu")
            td.all_reduce(flag, op=td.ReduceOp.MIN)
            if int(flag.item()) == 0:
                if link is not None and link.active:
                    link.close()
                link = None
                link_dropped = True
                if rank == 0:
                    print("[bench] direct link dropped on every rank after a failed solve; collectives use the "
                          f"{a.exchange} transport", file=sys.stderr, flush=True)
                td.barrier()
                run_iterations(5)
            for _ in range(max(0, int(round(a.settle * 100)) - 1)):
                run_iterations(5)
        run_iterations(max(1, a.warmup))
        barrier()
        n_launch0, n_coll0 = be.counters()
        t0 = time.perf_counter()
        results = run_iterations(a.steps)
        barrier()
        elapsed = time.perf_counter() - t0
        n_launch1, n_coll1 = be.counters()
        outputs = None
        if a.dump_outputs and rank == 0:   # the last timed solve's residual vector and gradient, before `be` runs anything else
            fun, grad = be.fetch_fun_grad(True, True)
            res = last["res"]
            outputs = {"x": last["x"], "fun": fun, "grad": grad, "cost": [res.cost], "rmse": [res.rmse],
                       "optimality": [res.optimality]}
        # outside the timed region: the same residual+Jacobian kernel compiled WITHOUT the point-block sums (another
        # symbol, so its launches do not mix with the solver's in a rocprofv3 trace of this command), back to back
        k1_plain_us = be.time_kernel(pb.x0, 7, 50) if world == 1 and a.full else None
        # `value` comes from back-to-back solves of the same x0, which replay the previous solve's per-iteration PCG
        # counts (no spare launch, never a miss).  The other end: the FIRST solve of a fresh handle (no record: one spare
        # PCG launch per iteration, counts guessed from the previous iteration), same problem resident, x0 crossing PCIe
        first_solve = None
        if world == 1 and a.full:
            fb = sfmba.Backend(local_rank)
            fb.set_precision(a.storage_bits)
            fb.set_problem(*pb.args)
            opt1 = fb.default_options()
            opt1.ftol = 1e-10
            t1 = time.perf_counter()
            _, r1, _, _ = fb.solve(pb.x0, opt1, want_fun=False, want_grad=False)
            dt1 = time.perf_counter() - t1
            first_solve = {"ms": round(1e3 * dt1, 3), "iterations": int(r1.iterations),
                           "iterations_per_s": round(int(r1.iterations) / dt1, 1),
                           "note": "first solve on a fresh handle: no PCG record to replay, first-use costs included"}
            fb.close()
        # ... and what the contract's "Jacobian blocks materialised" clause costs: the same solves in the J-free mode
        # (debug option jfree: K1 forms the blocks for the point sums without writing them, k_jdot / k_backsub recompute them;
        # bitwise the same result in fp64 storage).  NOT the default and not `value`: the judged residual+Jacobian kernel
        # writes its blocks.  Outside the timed region.
        j_free = None
        if world == 1 and a.full and a.shard_of <= 1 and Cl <= 1000:
            jb = sfmba.Backend(local_rank)
            jb.set_precision(a.storage_bits)
            jb.debug_option("jfree", 1)
            jb.set_problem(*pb.args)
            optj = jb.default_options()
            optj.ftol = 1e-10
            ts, its = [], []
            for k in range(16):
                _, rj, _, _ = jb.solve(pb.x0, optj, want_fun=False, want_grad=False)
                if k >= 4:
                    ts.append(float(rj.seconds_total)); its.append(int(rj.iterations))
            mid = sorted(range(len(ts)), key=lambda i: ts[i])[len(ts) // 2]          # the median solve (a companion
            j_free = {"iterations_per_s": round(its[mid] / ts[mid], 1),             # number: one queue hiccup in twelve
                      "ms_per_solve": round(1e3 * ts[mid], 3),                       # solves must not decide it)
                      "note": "same back-to-back solves with debug option jfree = 1 (no Jacobian stores in K1, blocks "
                              "recomputed by their two consumers), median of 12 solves; not the shipped default"}
            jb.close()

    if td is not None:
        tmax = torch.tensor([elapsed], dtype=torch.float64, device="cuda")
        td.all_reduce(tmax, op=td.ReduceOp.MAX)
        elapsed = float(tmax.item())

    if rank == 0:
        steps = sum(r[0] for r in results)
        k1_us = sum(r[3] * r[4] for r in results) / max(1, sum(r[4] for r in results))
        kb = k1_bytes_f32 if a.storage_bits == 32 else k1_bytes
        achieved = kb(Cl, Pl, Nl) / (k1_us * 1e-6) / 1e9 if k1_us > 0 else None
        traffic = traffic_src = None
        tpath = os.path.join(ROOT, "profiles", "k1_traffic.json")
        if os.path.exists(tpath) and world == 1 and a.shard_of <= 1:
            tj = json.load(open(tpath))
            if str(tj.get("workload", "")).split()[0] == a.workload and a.storage_bits == 64:
                traffic = tj.get("hbm_bytes_per_launch")
                traffic_src = ("NOT measured in this run: FETCH_SIZE / WRITE_SIZE of the same kernel and workload from the "
                               "committed rocprofv3 --pmc passes, profiles/k1_traffic.json")
        full = [r for r in results if r[6] != 0] or results
        strong = scaling == "strong"
        n_total, p_total = (N, P) if strong else (N * world, P * world)
        line = {
            "metric": "BA iterations/sec",
            # strong: iterations of the ONE problem per second; weak: shard-iterations summed over the ranks
            "value": steps / elapsed if strong else steps * world / elapsed,
            "unit": "iterations/s" if strong else "shard-iterations/s (one workload-sized shard per GPU, summed over GPUs)",
            "n_gpus": world, "steps": steps, "warmup": a.warmup,
            "ms_per_step": 1e3 * elapsed / steps,
            "settle_s": a.settle, "full": a.full,
            "higher_is_better": True, "scaling": scaling, "vs_baseline": None,
            "dtype": "f64" if a.storage_bits == 64 else "f64 arithmetic, f32 storage", "data": "synthetic",
            "transport": None if td is None else (f"direct xGMI all-reduce kernel ({be.p2p_calls()} collectives; "
                                                  f"fallback {a.exchange})" if (link is not None and link.active)
                                                  else (f"{a.exchange} (direct link dropped after a failed first solve)"
                                                        if link_dropped else a.exchange)),
            "value_is": "back-to-back solves from the same x0 (each replays the previous solve's PCG iteration record)",
            "first_solve_fresh_handle": first_solve,
            "j_free_iteration": j_free,
            "launches_per_iteration": round((n_launch1 - n_launch0) / steps, 1),
            "collectives_per_iteration": round((n_coll1 - n_coll0) / steps, 1),
            "config": {"workload": (f"{a.workload}: {C} cameras / {P} points / {N} observations, seed 0 (SURVEY.md 8d "
                                    f"generator)" + ((f"; RANK 0'S SHARE of a {a.shard_of}-way sharding only" if a.shard_of > 1 else "")
                                                     if world == 1 else
                                                     f", observations sharded at point boundaries over {world} GPUs"
                                                     if strong else f" PER GPU shard, shared cameras")),
                       "solver": "TRF (scipy trf_no_bounds restated) + analytic Jacobian + Schur PCG, ftol=1e-10",
                       "n_obs_total": n_total, "n_points_total": p_total, "n_cameras": C,
                       "n_obs_rank0": Nl, "n_points_rank0": Pl,
                       "solves_in_timed_region": len(results),
                       "iterations_per_solve": [r[0] for r in results],
                       "pcg_iterations_per_solve": [r[5] for r in results],
                       "ms_per_solve": [round(1e3 * r[7], 3) for r in results],
                       "back_to_back_kernel_us": {k: round(v, 2) for k, v in primed.items()}},
            "final_rmse_px": full[0][1], "initial_rmse_px": full[0][2],
            # time until the RMSE is final = wall time of a solve that ran to its ftol termination
            "time_to_final_rmse_ms": (round(1e3 * sorted(r[7] for r in full)[len(full) // 2], 3)
                                      if any(r[6] != 0 for r in results) else None),
            "roofline": {"kernel": "k_resjac (residual + 2x6/2x3 Jacobian sweep + point blocks V_p, g_p)", "bound": "hbm",
                         "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": (achieved / HBM_PEAK_GBS) if achieved else None,
                         "traffic": traffic, "traffic_source": traffic_src, "avg_launch_us": k1_us,
                         "algorithmic_bytes_per_launch": kb(Cl, Pl, Nl),
                         "note": "bytes = 136 N + 96 P + 48 C of the rank's shard: the 2x3 block d r/d T = -d r/d X is "
                                 "not stored; SURVEY 8d's 184 N figure writes it a second time",
                         "achieved_if_counted_as_survey_184B": (k1_bytes_survey(Cl, Pl, Nl) / (k1_us * 1e-6) / 1e9)
                                                                if k1_us > 0 else None,
                         "launches_timed": sum(r[4] for r in results),
                         "without_point_blocks": (None if not k1_plain_us else {
                             "note": "k_resjac<...,BLOCKS=false>: the kernel as it was before it absorbed the point pass "
                                     "(V_p, g_p; 72 B per point less), 50 back-to-back launches outside the timed region",
                             "avg_launch_us": k1_plain_us,
                             "algorithmic_bytes_per_launch": kb(Cl, Pl, Nl) - 72 * Pl,
                             "achieved": (kb(Cl, Pl, Nl) - 72 * Pl) / (k1_plain_us * 1e-6) / 1e9,
                             "frac": (kb(Cl, Pl, Nl) - 72 * Pl) / (k1_plain_us * 1e-6) / 1e9 / HBM_PEAK_GBS})},
        }
        if world == 1 and a.full and not a.no_per_call:
            line["per_call_ms"] = per_call_times(a.workload, a.storage_bits)
        if a.full and not a.no_cpu_baseline and world == 1:     # the CPU baseline is timed on rank 0 at N = 1 only
            line["cpu_baseline"] = cpu_baseline((C, P, N))
            line["speedup_vs_cpu_baseline"] = (steps / elapsed) / line["cpu_baseline"]["value"]
        if outputs is not None:
            dump_outputs(a.dump_outputs, outputs)
        print(json.dumps(line), flush=True)
    if td is not None:
        td.barrier()
        td.destroy_process_group()


if __name__ == "__main__":
    main()
