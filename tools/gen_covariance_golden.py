#!/usr/bin/env python3
"""Writes tests/golden/covariance_bounds.json on the CPU (numpy only): for every case of tests/covariance_ref.py the
spread between the reference's two routes (what the GPU is held to, times `factor`), the smallest relative pivot of the
gauged S and of the points, and seven-th / eighth-smallest over largest eigenvalue of the unheld S.  A case whose smallest
pivot lies within 100x of rank_tol / point_tol, or whose unheld S does not show seven null eigenvalues, is rejected.

    python tools/gen_covariance_golden.py            # all cases -> tests/golden/covariance_bounds.json
    python tools/gen_covariance_golden.py --only c3  # print one case's record, write nothing
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "sfm-python_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import covariance_ref as ref  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    names = [a.only] if a.only else list(ref.CASES)
    cases = {}
    for name in names:
        rec = ref.case_bounds(name)
        why = ref.accept(name, rec)
        if why:
            raise SystemExit(f"case {name} rejected: {why}")
        cases[name] = rec
        print(name, json.dumps(rec))
    if a.only:
        return
    out = {"factor": ref.FACTOR, "rank_tol": ref.RANK_TOL, "point_tol": ref.POINT_TOL,
           "measure": "max |a_ij - b_ij| / sqrt(b_ii b_jj) between route A (inverse of the whole reduced J^T J) and route B "
                      "(Schur + Cholesky)", "cases": cases}
    with open(ref.BOUNDS_PATH, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
