"""Timing of the covariance call at the 11- and the 21-camera case of its tests: the kernel group of
one call with the default options, point sweep included (sfmba_time_kernel which = 18), one Backend.covariance call end to
end, and one sfmba_solve on the same problem beside them for scale.  There is no target.  Usage: python tools/cov_timing.py

The kernel figure is the median of ROUNDS windows of REPS back-to-back groups between HIP events (as tools/stats_timing.py
takes its figures); min and max of the windows are the scatter.  The end-to-end figures are medians of 7 calls."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "sfm-python_amd"), os.path.join(ROOT, "tests")]
import numpy as np

import covariance_ref as cr
import sfmba

ROUNDS, REPS = 9, 20


def main():
    be = sfmba.Backend(0)
    for name in ("c11", "c21"):
        c = cr.case(name)
        C, P, ci = c["args"][0], c["args"][1], c["args"][2]
        be.set_precision(64)
        be.set_fixed_cameras(())
        be.set_problem(*c["args"])
        be.time_kernel(c["x"], 18, 3)                                      # warm-up: code objects, buffers, LDS opt-in
        be.debug_option("cov_lds", 1)
        be.time_kernel(c["x"], 18, 3)
        win = {0: [], 1: []}
        for _ in range(ROUNDS):                                            # the two forms of the point sweep in turn
            for lds in (0, 1):
                be.debug_option("cov_lds", lds)
                win[lds].append(be.time_kernel(c["x"], 18, REPS))
        be.debug_option("cov_lds", -1)
        print(f"{name}: {C} cameras, {P} points, {len(ci)} observations", flush=True)
        for lds, label in ((0, "Sigma_cc read from L2"), (1, "Sigma_cc staged in LDS")):
            v = np.array(win[lds])
            print(f"  which=18 covariance kernels, {label:22s} median {np.median(v):9.2f} us  min {v.min():9.2f}  max {v.max():9.2f}",
                  flush=True)
        for label, kw in (("marginal, all arrays", dict(want_full=True)), ("marginal, cameras only", dict(want_points=False)),
                          ("conditional, all arrays", dict(kind="conditional"))):
            be.covariance(c["x"], **kw)
            t = []
            for _ in range(7):
                t0 = time.perf_counter()
                cov = be.covariance(c["x"], **kw)
                t.append(time.perf_counter() - t0)
            print(f"  covariance, {label:24s} median {1e3 * np.median(t):8.3f} ms  min {1e3 * min(t):8.3f}  max {1e3 * max(t):8.3f}"
                  f"   (status {cov.status}, sigma2 {cov.sigma2:.4f})", flush=True)
        prof = be.covariance(c["x"], profile=1)
        print(f"  covariance, profile = 1: kernel_us {prof.kernel_us:9.2f} (with the two read-backs between its stages)", flush=True)
        pb = sfmba.make_problem(C, P, len(ci), seed={"c11": 2, "c21": 3}[name])
        opt = be.default_options()
        opt.ftol = 1e-10
        be.solve(pb.x0, opt)
        t = []
        for _ in range(7):
            t0 = time.perf_counter()
            _, res, _, _ = be.solve(pb.x0, opt)
            t.append(time.perf_counter() - t0)
        print(f"  one sfmba_solve from x0 (ftol 1e-10, {res.iterations} iterations) median {1e3 * np.median(t):8.3f} ms  "
              f"min {1e3 * min(t):8.3f}  max {1e3 * max(t):8.3f}", flush=True)
    be.close()


main()
