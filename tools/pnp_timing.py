"""Timings of the robust resection: k_pnp_ransac + k_pnp_finish over every camera
(sfmba_time_kernel which = 17, default options: 256 hypotheses per camera) beside the plain DLT resection on the same
problem (which = 16), one Backend.resect_ransac and one Backend.resect call end to end, and the cost per hypothesis and
wave to be read against section 18's.  Problems: cfg2 (11 cameras), one camera x 2000 observations, cfg4 (1000 cameras,
about 1000 observations each); for the one-camera problem also the numpy restatement on the CPU.  No threshold is attached.
Usage: python tools/pnp_timing.py [cfg2 one cfg4]

Every kernel figure is the median of ROUNDS windows of REPS back-to-back launches between HIP events, the two kernels
taken in turn inside every round; min and max of the windows are the scatter."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "sfm-python_amd"), os.path.join(ROOT, "tests")]
import numpy as np

import sfmba

ROUNDS, REPS, H = 9, 20, 256


def one_camera(n=2000, seed=3):
    """One camera, n points of its own 4..9 units in front of it, 0.5 px of noise, 30 % of the pixels displaced."""
    rng = np.random.default_rng(seed)
    K = sfmba.K_SCEAUX.copy()
    cam = np.stack([rng.uniform(-1.8, 1.8, n), rng.uniform(-1.3, 1.3, n), rng.uniform(4.0, 9.0, n)], axis=1)
    uv = cam @ K.T
    uv = uv[:, :2] / uv[:, 2:3] + 0.5 * rng.normal(size=(n, 2))
    bad = rng.random(n) < 0.3
    uv[bad] += rng.uniform(20.0, 200.0, (int(bad.sum()), 2))
    x = np.concatenate([np.zeros(6), cam.ravel()])
    return x, (1, n, np.zeros(n, dtype=np.int64), np.arange(n, dtype=np.int64), uv, K)


def main():
    be = sfmba.Backend(0)
    for name in sys.argv[1:] or ["cfg2", "one", "cfg4"]:
        if name == "one":
            x, args = one_camera()
        else:
            pb = sfmba.make_config(name)
            x, args = pb.x0, pb.args
        C, N = args[0], len(args[2])
        be.set_problem(*args)
        for which in (16, 17):
            be.time_kernel(x, which, 3)                          # warm-up: code objects, buffers
        win = {16: [], 17: []}
        for _ in range(ROUNDS):
            for which in win:
                win[which].append(be.time_kernel(x, which, REPS))
        print(f"{name}: {C} cameras, {N} observations, {H} hypotheses per camera", flush=True)
        for which, label in ((16, "k_resect (DLT + refinement)"), (17, "k_pnp_ransac + k_pnp_finish")):
            v = np.array(win[which])
            print(f"  which={which} {label:30s} median {np.median(v):10.2f} us  min {v.min():10.2f}  max {v.max():10.2f}", flush=True)
        # hypotheses are solved 64 at a time by a wave: waves needed = ceil(H / 64) per camera, spread over the device
        med = float(np.median(win[17]))
        print(f"  per hypothesis: {1e3 * med / (C * H):.1f} ns of the launch pair's time; the batch's {C * H} hypotheses "
              f"are {C * ((H + 63) // 64)} wave-rounds of 64", flush=True)
        for label, call in (("resect_ransac, all arrays", lambda: be.resect_ransac(x, max_iters=H)),
                            ("resect, all arrays", lambda: be.resect(x))):
            call()
            t = []
            for _ in range(7):
                t0 = time.perf_counter()
                r = call()                                       # returns after the downloads: synchronised
                t.append(time.perf_counter() - t0)
            print(f"  {label:30s} median {1e3 * np.median(t):8.3f} ms  min {1e3 * min(t):8.3f}  max {1e3 * max(t):8.3f}   "
                  f"({r.n_ok} of {C} cameras OK)", flush=True)
        if name == "one":
            import pnp_ransac_ref as pr
            t0 = time.perf_counter()
            ref = pr.resect_ransac(x, args, max_iters=H)
            print(f"  numpy restatement on the CPU      {time.perf_counter() - t0:8.3f} s   ({int(ref['inliers'][0])} inliers; "
                  f"device {int(be.resect_ransac(x, max_iters=H).inliers[0])})", flush=True)
    be.close()


main()
