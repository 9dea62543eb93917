#!/usr/bin/env python
"""tests/golden/iteration_bounds.json: what the PCG of one outer iteration is off by between the reference's own two
precisions, for every case of tests/iteration_ref.py (PCG_CASES).  CPU only; nothing here comes from a device.

Rounding is amplified through the iterations of a conjugate-gradient solve, so no counted k bounds the camera step.  For
every case the iteration is replayed at x0 in plain float64 (the oracle's blocks, numpy's sums) up to the operands of the
PCG -- Dc, reg si_p^2, Minv -- and the PCG itself is then run twice on those operands: in longdouble on the longdouble
linearisation until its stop rule holds (that count is `iters`), and in float64 for the same number of iterations.
Recorded per case, with the largest over the camera blocks:
    dc        |dc64_c - dcld_c|_inf / |dcld_c|_inf
    identity  |r64_c + (S x64)_c - b_c|_inf / |b_c|_inf   (the product and b in longdouble)
    rz        the relative error of rz0 and of the last rz
The GPU test holds the device to `factor` = 100 times these, the convention of the other *_bounds.json files.

Two conditions keep the iteration count from being a coin toss, asserted here and by tests/test_host_iteration.py: in the
longdouble replay rz / (tol2 rz0) at `iters` and at `iters - 1` lies at least MARGIN = 1e-6 away from 1, and no case ends in
a breakdown (done == 3) or at the iteration cap.

    python tools/gen_iteration_golden.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "sfm-python_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

FACTOR = 100.0


def main():
    import iteration_ref as ir
    from oracle import ba_oracle as orc
    cases = {}
    for name in ir.PCG_CASES:
        m = ir.measure_pcg_case(name, orc)
        assert m["done"] == 1, (name, m)
        assert m["iters"] >= 1 and abs(m["margin_at"] - 1) >= ir.MARGIN and abs(m["margin_before"] - 1) >= ir.MARGIN, (name, m)
        assert m["margin_at"] < 1 < m["margin_before"] or m["iters"] == 1, (name, m)
        cases[name] = m
        print(f"{name}: {m['iters']} iterations, dc {m['dc']:.3e}, identity {m['identity']:.3e}, rz {m['rz']:.3e}, "
              f"rz / (tol2 rz0) {m['margin_before']:.3g} -> {m['margin_at']:.3g}")
    with open(ir.BOUNDS_FILE, "w") as f:
        json.dump({"factor": FACTOR, "margin": ir.MARGIN, "cases": cases}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
