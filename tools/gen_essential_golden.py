"""Writes tests/golden/essential_bounds.json: what the numpy restatement (tests/essential_ref.py) itself reaches on the
inputs of tests/test_gpu_essential.py, on the CPU.  The GPU tests hold the device to multiples of these figures.
Usage: python tools/gen_essential_golden.py"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import essential_ref as er  # noqa: E402
import two_view_ref as tv  # noqa: E402

E2E_H, E2E_SEED = 200, 5
PAIR_H, PAIR_SEED = 60, 9


def main():
    K = er.K_TEST
    # the backward errors of the restatement's polished candidate nearest the truth over the 200 noise-free five-pair samples
    p1, p2, ptr, Et = er.exact_cases()
    epi, trace = 0.0, 0.0
    for e in range(len(Et)):
        a, b = p1[ptr[e]:ptr[e] + 5], p2[ptr[e]:ptr[e] + 5]
        for route in ("eigh", "svd"):
            Es, _ = er.candidates(a, b, K, route)
            E = er.polish(a, b, K, Es[er.nearest(Es, Et[e])[0]], route)
            x, y = er.backward_errors(E, K, a, b)
            epi, trace = max(epi, x), max(trace, y)
    # the pose of the restatement's RANSAC on the noisy scene
    q1, q2, R, t = er.noisy_scene()
    est = er.ransac_edge(q1, q2, K, er.draw_samples5(E2E_SEED, 0, E2E_H, len(q1)), er.THRESHOLD)
    assert est["status"] == er.OK
    m = est["mask"]
    pose = tv.recover_pose_edge(est["E"], q1[m], q2[m], K)
    assert pose["status"] == tv.OK
    rot, tdir = er.pose_errors(pose["R"], pose["t"], R, t)
    choice = er.initial_pair_choice(er.pair_edges(), PAIR_H, PAIR_SEED)
    out = dict(backward=dict(epipolar=epi, trace=trace),
               end_to_end=dict(H=E2E_H, seed=E2E_SEED, inliers=int(est["inliers"]), rotation_rad=rot, translation_rad=tdir),
               initial_pair=dict(H=PAIR_H, seed=PAIR_SEED, index=choice))
    path = os.path.join(ROOT, "tests", "golden", "essential_bounds.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
