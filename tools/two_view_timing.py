"""Timings of the two-view calls: sfmba_fundamental_ransac (k_fund_ransac + k_fund_finish, refit on)
and sfmba_recover_pose (k_recover_pose) from their own `kernel_us` (profile = 1: HIP events round the call's launches), and
one call of each end to end, on three batches at H = 1000 hypotheses: 1 edge x 2000 pairs, 55 edges x 500 pairs (every pair
of 11 cameras) and 4950 edges x 300 pairs (every pair of 100 images).  Beside the 1-edge case: the reference's CPU time for
the same shape as tools/gen_two_view_golden.py measured it (tests/golden/two_view_bounds.json).  No speed threshold is
attached: no parent exists to compare with.  Usage: python tools/two_view_timing.py [1x2000 55x500 4950x300]

Every kernel figure is the median of ROUNDS calls, the two calls taken in turn inside every round (so drift of the box hits
them alike); min and max are the scatter."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "sfm-python_amd"), os.path.join(ROOT, "tests")]
import numpy as np

import sfmba
import two_view_ref as tv

ROUNDS, H = 9, 1000
SHAPES = {"1x2000": (1, 2000), "55x500": (55, 500), "4950x300": (4950, 300)}


def main():
    be = sfmba.Backend(0)
    K = sfmba.K_SCEAUX
    bounds = json.load(open(os.path.join(ROOT, "tests", "golden", "two_view_bounds.json")))
    for name in sys.argv[1:] or list(SHAPES):
        E, n = SHAPES[name]
        rng = np.random.default_rng(1)
        scenes = [tv.make_pairs(rng, n, K, noise=0.3, outliers=0.25) for _ in range(min(E, 55))]     # (reused round robin)
        p1 = np.concatenate([scenes[e % len(scenes)][0] for e in range(E)])
        p2 = np.concatenate([scenes[e % len(scenes)][1] for e in range(E)])
        ptr = np.arange(E + 1, dtype=np.int64) * n
        kw = dict(edge_ptr=ptr, threshold=1.0, max_iters=H, seed=1, refit=1, profile=1)
        est = be.fundamental_ransac(p1, p2, **kw)                             # warm-up: code objects, buffers
        Es = np.einsum("ji,ejk,kl->eil", K, est.F_refit, K)
        be.recover_pose(Es, p1, p2, K, edge_ptr=ptr, pair_use=est.inlier_mask, profile=1)
        us = {"ransac": [], "pose": []}
        wall = {"ransac": [], "pose": []}
        for _ in range(ROUNDS):
            t0 = time.perf_counter()
            est = be.fundamental_ransac(p1, p2, **kw)
            wall["ransac"].append(time.perf_counter() - t0)
            us["ransac"].append(est.kernel_us)
            t0 = time.perf_counter()
            pose = be.recover_pose(Es, p1, p2, K, edge_ptr=ptr, pair_use=est.inlier_mask, profile=1)
            wall["pose"].append(time.perf_counter() - t0)
            us["pose"].append(pose.kernel_us)
        print(f"{name}: {E} edges x {n} pairs, H = {H}; {est.n_ok} edges with an F, {pose.n_ok} with a pose, "
              f"{float(est.inliers.mean()):.1f} inliers per edge", flush=True)
        for key, label in (("ransac", "k_fund_ransac + k_fund_finish"), ("pose", "k_recover_pose")):
            v, w = np.array(us[key]), 1e3 * np.array(wall[key])
            print(f"  {label:30s} median {np.median(v):11.2f} us  min {v.min():11.2f}  max {v.max():11.2f}   "
                  f"call end to end median {np.median(w):9.3f} ms  min {w.min():9.3f}  max {w.max():9.3f}", flush=True)
        if name == "1x2000":
            ref = bounds["reference_cpu_seconds_1x2000_H1000"]
            print(f"  the reference's estimate_fundamental_matrix_ransac on this shape, CPU, as the fixtures' generator measured it: "
                  f"{1e3 * ref:.1f} ms ({1e6 * ref / np.median(us['ransac']):.0f} x the kernels)", flush=True)
    be.close()


main()
