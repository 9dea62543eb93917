"""tests/golden/tri_ransac_bounds.json: what the tests of sfmba_triangulate_ransac take from the CPU, measured with the
numpy restatement (tests/tri_ransac_ref.py) on the tests' own inputs and nothing else -- no device, no library.

Per case of tri_ransac_ref.CASES: the number of hypotheses and the share the restatement flags `close` (the tests require
at most CLOSE_CAP), the planted-truth recovery of the contaminated tracks, and two distances with the bound the kernel is
held to, FACTOR times the measured maximum (the project's factor for "same algorithm, different rounding order":
fused multiply-adds, rotation order, summation order): the pair point by the interface's route (A^T A, cyclic Jacobi)
against numpy.linalg.svd of the same four rows over every valid hypothesis, and the n-view linear point of every inlier
set against the SVD of its rows.  Relative to max(1, |X|_inf), as tests/golden/triangulate_bounds.json.

    python tools/gen_tri_ransac_golden.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "sfm-python_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

FACTOR = 100.0
CLOSE_CAP = 0.05


def main():
    import tri_ransac_ref as trr
    rec = dict(factor=FACTOR, close_cap=CLOSE_CAP, close_relative=trr.CLOSE, cases={})
    for name in trr.CASES:
        m, _ = trr.measure_case(name)
        m["pair_bound_rel"] = FACTOR * m["pair_measured_rel"]
        m["final_linear_bound_rel"] = FACTOR * m["final_linear_measured_rel"]
        rec["cases"][name] = m
        print(name, json.dumps(m))
    with open(os.path.join(ROOT, "tests", "golden", "tri_ransac_bounds.json"), "w") as f:
        json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
