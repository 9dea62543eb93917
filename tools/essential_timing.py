"""Timings of the essential-matrix call: sfmba_essential_ransac (k_ess_ransac + k_ess_finish) from
its own `kernel_us` (profile = 1: HIP events round the call's launches) and one call end to end, on two batches: a
graph-like one of 1000 edges x 300 pairs x 1000 hypotheses, and one edge of 4096 pairs (the most that is staged in LDS)
x 1000 hypotheses.  Beside each figure: sfmba_fundamental_ransac (refit off) on the same batch, in the same process, the
two calls taken in turn.  No threshold is attached: there is no earlier implementation and no reference code for E; the F
call is the yardstick only because the launch structure is shared (one wave per hypothesis; F: a 9x9 Jacobi plus n / 64
scoring rounds; E: the Jacobi, the 10 x 20 elimination, the roots, and n / 64 rounds against every candidate).
Usage: python tools/essential_timing.py [1000x300 1x4096]

Every figure is the median of ROUNDS warm calls; min and max are the scatter."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "sfm-python_amd"), os.path.join(ROOT, "tests")]
import numpy as np

import sfmba
import two_view_ref as tv

ROUNDS, H = 5, 1000
SHAPES = {"1000x300": (1000, 300), "1x4096": (1, 4096)}


def main():
    be = sfmba.Backend(0)
    K = sfmba.K_SCEAUX
    for name in sys.argv[1:] or list(SHAPES):
        E, n = SHAPES[name]
        rng = np.random.default_rng(1)
        scenes = [tv.make_pairs(rng, n, K, noise=0.3, outliers=0.25)[:2] for _ in range(min(E, 50))]    # (reused round robin)
        p1 = np.concatenate([scenes[e % len(scenes)][0] for e in range(E)])
        p2 = np.concatenate([scenes[e % len(scenes)][1] for e in range(E)])
        ptr = np.arange(E + 1, dtype=np.int64) * n
        kw = dict(edge_ptr=ptr, threshold=1.0, max_iters=H, seed=1, profile=1)
        calls = {"E": lambda: be.essential_ransac(p1, p2, K, want_hyp=True, **kw), "F": lambda: be.fundamental_ransac(p1, p2, **kw)}
        for call in calls.values():
            call()                                               # warm-up: code objects, buffers
        us, wall, last = {k: [] for k in calls}, {k: [] for k in calls}, {}
        for _ in range(ROUNDS):
            for key, call in calls.items():
                t0 = time.perf_counter()
                last[key] = call()                               # returns after the downloads: synchronised
                wall[key].append(time.perf_counter() - t0)
                us[key].append(last[key].kernel_us)
        roots = last["E"].hyp_roots
        print(f"{name}: {E} edges x {n} pairs, H = {H}; {last['E'].n_ok} edges with an E ({float(last['E'].inliers.mean()):.1f} inliers "
              f"per edge, {float(roots[roots >= 0].mean()):.2f} real roots per hypothesis), {last['F'].n_ok} with an F "
              f"({float(last['F'].inliers.mean()):.1f} inliers per edge)", flush=True)
        for key, label in (("E", "k_ess_ransac + k_ess_finish"), ("F", "k_fund_ransac + k_fund_finish")):
            v, w = np.array(us[key]), 1e3 * np.array(wall[key])
            print(f"  {label:32s} median {np.median(v):11.2f} us  min {v.min():11.2f}  max {v.max():11.2f}   "
                  f"call end to end median {np.median(w):9.3f} ms  min {w.min():9.3f}  max {w.max():9.3f}", flush=True)
        print(f"  per hypothesis and edge: E {1e3 * np.median(us['E']) / (E * H):.1f} ns, F {1e3 * np.median(us['F']) / (E * H):.1f} ns "
              f"of the launch pair's time", flush=True)
    be.close()


main()
