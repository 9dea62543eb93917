"""Timings of the reprojection statistics, of the triangulation (section 15) and of the resection
(section 16): the per-observation sweep (sfmba_time_kernel which = 13) beside the residual-only sweep (which = 1), the
per-point reduction (which = 14), k_triangulate over every track (which = 15) and k_resect over every camera (which = 16),
both with default options, with their algorithmic bytes, and one Backend.reprojection_stats, one Backend.triangulate and
one Backend.resect call end to end.  No speed threshold is attached to which = 15 and 16.  Usage: python tools/stats_timing.py [cfg2 cfg4 cfg5] [--bits 64|32]

Every kernel figure is the median of ROUNDS windows of REPS back-to-back launches between HIP events, the three kernels
taken in turn inside every round (so drift of the box hits them alike); min and max of the windows are the scatter."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "sfm-python_amd")]
import numpy as np

import sfmba

ROUNDS, REPS = 9, 40
HBM_PEAK = 8.0e12


def main():
    argv = sys.argv[1:]
    bits = 64
    if "--bits" in argv:
        k = argv.index("--bits")
        bits = int(argv[k + 1])
        del argv[k:k + 2]
    be = sfmba.Backend(0)
    be.set_precision(bits)
    px = 8 if bits == 32 else 16
    for cfg in argv or ["cfg2", "cfg4", "cfg5"]:
        C, P, N = sfmba.synthetic.CONFIGS[cfg]
        pb = sfmba.make_config(cfg)
        be.set_problem(*pb.args)
        # algorithmic bytes: index and pixel streams, every point and camera row once, the stores
        nbytes = {1: (8 + px) * N + 24 * P + 144 * C,                        # (as timed it stores no residual)
                  13: (8 + px) * N + 24 * P + 144 * C + 17 * N,               # err | depth pair + mask byte
                  14: (16 + 1 + 4 + 1) * N + (4 + 24 + 37) * P + 24 * C,      # pairs, masks, camera index | run offsets, point, results
                  15: (4 + px) * N + (4 + 24 + 52) * P + 96 * C,              # FIRST pass of a run (the 1 + iterations others hit L2):
                                                                              # camera index, pixel | run offset, point, results | R, T rows
                  16: (4 + 4 + px + 24) * N + (4 + 48 + 72) * C}              # FIRST pass of a slice: permutation entry, point index,
                                                                              # pixel, gathered point | slice offset, camera of x, results
        for which in nbytes:
            be.time_kernel(pb.x0, which, 5)                                   # warm-up: code objects, buffers
        win = {w: [] for w in nbytes}
        for _ in range(ROUNDS):
            for which in nbytes:
                win[which].append(be.time_kernel(pb.x0, which, REPS))
        print(f"{cfg}: {C} cameras, {P} points, {N} observations, {bits}-bit storage", flush=True)
        for which, name in ((1, "residual-only sweep"), (13, "per-observation sweep"), (14, "per-point reduction"),
                            (15, "triangulation"), (16, "resection")):
            v = np.array(win[which])
            med = float(np.median(v))
            print(f"  which={which:2d} {name:22s} median {med:9.2f} us  min {v.min():9.2f}  max {v.max():9.2f}  "
                  f"{nbytes[which] / 1e6:8.2f} MB  {nbytes[which] / med / 1e6:7.3f} TB/s  "
                  f"{nbytes[which] / med / 1e-6 / HBM_PEAK:5.3f} of HBM peak", flush=True)
        for want, label in ((("obs", "points", "cameras"), "all arrays"), (("points",), "points only"), ((), "summary only")):
            be.reprojection_stats(pb.x0, want=want)
            t = []
            for _ in range(7):
                t0 = time.perf_counter()
                st = be.reprojection_stats(pb.x0, want=want)                  # returns after the downloads: synchronised
                t.append(time.perf_counter() - t0)
            print(f"  reprojection_stats, {label:12s} median {1e3 * np.median(t):8.3f} ms  min {1e3 * min(t):8.3f}  "
                  f"max {1e3 * max(t):8.3f}   (mean error {st.mean_error_px:.3f} px)", flush=True)
        be.triangulate(pb.x0)
        t = []
        for _ in range(7):
            t0 = time.perf_counter()
            tri = be.triangulate(pb.x0)
            t.append(time.perf_counter() - t0)
        print(f"  triangulate, all arrays        median {1e3 * np.median(t):8.3f} ms  min {1e3 * min(t):8.3f}  "
              f"max {1e3 * max(t):8.3f}   ({tri.n_ok} of {P} points OK, {float(tri.iters.mean()):.2f} trial points per track)",
              flush=True)
        be.resect(pb.x0)
        t = []
        for _ in range(7):
            t0 = time.perf_counter()
            rs = be.resect(pb.x0)
            t.append(time.perf_counter() - t0)
        print(f"  resect, all arrays             median {1e3 * np.median(t):8.3f} ms  min {1e3 * min(t):8.3f}  "
              f"max {1e3 * max(t):8.3f}   ({rs.n_ok} of {C} cameras OK, {float(rs.iters.mean()):.2f} trial poses per camera)",
              flush=True)
    be.close()


main()
