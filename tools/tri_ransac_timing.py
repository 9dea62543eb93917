"""Timings of the robust triangulation: the kernels of sfmba_triangulate_ransac (sfmba_time_kernel
which = 19: k_tri_ransac, then k_triangulate over its mask; default options, 64 pairs at most) beside k_triangulate over
every observation (which = 15) on the bench problem (cfg4: 1000 cameras, 100 k points, 1 M observations), and entry 19
broken down by track-length class: problems whose tracks all have n views (100 k tracks of n = 2, 4, 10, 12; 20 k of
n = 31, 32, 64), cameras
and points of cfg4.  No threshold is attached.
Usage: python tools/tri_ransac_timing.py [cfg4 classes]

Every figure is the median of ROUNDS windows of REPS back-to-back launches between HIP events, the two entries taken in
turn inside every round; min and max of the windows are the scatter."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "sfm-python_amd"), os.path.join(ROOT, "tests")]
import numpy as np

import sfmba

ROUNDS, REPS = 9, 10
CLASSES = (2, 4, 10, 12, 31, 32, 64)


def windows(be, x):
    for which in (15, 19):
        be.time_kernel(x, which, 2)                              # warm-up: code objects, buffers
    win = {15: [], 19: []}
    for _ in range(ROUNDS):
        for which in win:
            win[which].append(be.time_kernel(x, which, REPS))
    return {w: np.array(v) for w, v in win.items()}


def report(name, args, win):
    P, N = args[1], len(args[2])
    n = np.bincount(np.asarray(args[3]), minlength=P)
    hyp = int(np.minimum(n * (n - 1) // 2, 64).sum())
    print(f"{name}: {args[0]} cameras, {P} points, {N} observations, mean track {N / P:.1f}, {hyp} hypotheses", flush=True)
    for which, label in ((15, "k_triangulate"), (19, "k_tri_ransac + k_triangulate")):
        v = win[which]
        print(f"  which={which} {label:30s} median {np.median(v):10.2f} us  min {v.min():10.2f}  max {v.max():10.2f}", flush=True)
    med = float(np.median(win[19]) - np.median(win[15]))
    print(f"  entry 19 less entry 15: {med:.1f} us = {1e3 * med / max(hyp, 1):.2f} ns per hypothesis", flush=True)


def class_problem(pb, n, n_tracks=100000, seed=5):
    """n_tracks tracks of exactly n views of distinct cameras: cameras and points of pb, pixels their projections + 0.5 px."""
    from oracle import ba_oracle as orc
    rng = np.random.default_rng(seed)
    C, P = pb.n_cameras, n_tracks
    ci = np.argsort(rng.random((P, C)), axis=1)[:, :n].ravel().astype(np.int64)
    pi = np.repeat(np.arange(P, dtype=np.int64), n)
    x = np.concatenate([pb.x_true[:6 * C], pb.x_true[6 * C:6 * C + 3 * P]])
    proj = orc.compute_residuals(x, C, P, ci, pi, np.zeros((len(ci), 2)), pb.K).reshape(-1, 2)
    return x, (C, P, ci, pi, proj + rng.normal(0.0, 0.5, proj.shape), pb.K)


def main():
    be = sfmba.Backend(0)
    what = sys.argv[1:] or ["cfg4", "classes"]
    pb = sfmba.make_config("cfg4")
    if "cfg4" in what:
        be.set_problem(*pb.args)
        report("cfg4", pb.args, windows(be, pb.x_true))
        t = []
        for _ in range(5):
            t0 = time.perf_counter()
            r = be.triangulate_ransac(pb.x_true)
            t.append(time.perf_counter() - t0)
        print(f"  triangulate_ransac, all arrays   median {1e3 * np.median(t):8.3f} ms   ({r.n_ok} of {pb.args[1]} points OK)", flush=True)
    if "classes" in what:
        for n in CLASSES:
            x, args = class_problem(pb, n, n_tracks=100000 if n <= 12 else 20000)
            be.set_problem(*args)
            report(f"n = {n}", args, windows(be, x))
    be.close()


if __name__ == "__main__":
    main()
