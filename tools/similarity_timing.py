"""Timings of the similarity call: sfmba_similarity_ransac (k_sim_ransac + k_sim_finish, refit on)
from its own `kernel_us` (profile = 1: HIP events round the call's launches) and one call end to end, on two batches: 64
sets x 2000 pairs x 1000 hypotheses, and one set of 300 pairs x 1000 hypotheses.  Beside them the wall time of the numpy
restatement (tests/similarity_ref.py: ransac_set) on ONE set of the batch with the same samples -- a yardstick of what the
work is, not a competitor: it is a Python loop over the hypotheses.  No threshold is attached: there is no earlier
implementation.  Usage: python tools/similarity_timing.py [64x2000 1x300]

Every device figure is the median of ROUNDS warm calls; min and max are the scatter."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "sfm-python_amd"), os.path.join(ROOT, "tests")]
import numpy as np

import sfmba
import similarity_ref as sr

ROUNDS, H, THR = 5, 1000, 0.05
SHAPES = {"64x2000": (64, 2000), "1x300": (1, 300)}


def main():
    be = sfmba.Backend(0)
    for name in sys.argv[1:] or list(SHAPES):
        E, n = SHAPES[name]
        rng = np.random.default_rng(1)
        sets = [sr.similar_sets(rng, n, noise=0.01, outliers=0.25)[:2] for _ in range(E)]
        src, dst = np.concatenate([s[0] for s in sets]), np.concatenate([s[1] for s in sets])
        ptr = np.arange(E + 1, dtype=np.int64) * n
        kw = dict(set_ptr=ptr, threshold=THR, max_iters=H, seed=1, refit=1, profile=1)
        be.similarity_ransac(src, dst, **kw)                     # warm-up: code objects, buffers
        us, wall = [], []
        for _ in range(ROUNDS):
            t0 = time.perf_counter()
            last = be.similarity_ransac(src, dst, **kw)          # returns after the downloads: synchronised
            wall.append(time.perf_counter() - t0)
            us.append(last.kernel_us)
        t0 = time.perf_counter()
        ref = sr.ransac_set(sets[0][0], sets[0][1], sr.draw_samples3(1, 0, H, n), THR, refit=True)
        t_ref = time.perf_counter() - t0
        v, w = np.array(us), 1e3 * np.array(wall)
        print(f"{name}: {E} sets x {n} pairs, H = {H}; {last.n_ok} sets with a similarity "
              f"({float(last.refit_inliers.mean()):.1f} refit inliers per set; the restatement's set 0: {ref['refit_inliers']}, "
              f"the device's: {int(last.refit_inliers[0])})", flush=True)
        print(f"  k_sim_ransac + k_sim_finish      median {np.median(v):11.2f} us  min {v.min():11.2f}  max {v.max():11.2f}   "
              f"call end to end median {np.median(w):9.3f} ms  min {w.min():9.3f}  max {w.max():9.3f}", flush=True)
        print(f"  per hypothesis and set: {1e3 * np.median(v) / (E * H):.1f} ns, per hypothesis and pair: "
              f"{1e6 * np.median(v) / (E * H * n):.1f} ps of the launch pair's time", flush=True)
        print(f"  numpy restatement, ONE set, the same {H} samples: {1e3 * t_ref:9.1f} ms wall", flush=True)
    be.close()


main()
