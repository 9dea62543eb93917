#!/usr/bin/env python
"""Fixtures of the two-view tests: tests/golden/two_view_cases.npz and tests/golden/two_view_bounds.json.

Runs only where the reference checkout exists (never on the GPU box): its teaching implementations of
cv2.findFundamentalMat and cv2.recoverPose, cv2_lite/fundamental_matrix_estimation.py and cv2_lite/recover_pose.py, need
numpy + scipy only and are imported from the checkout given with --reference.  Outputs are data only: seeded synthetic
pixel pairs, recorded sample sets, and what the reference's functions return for them.  No reference source is written
anywhere.

RANSAC cases: n = 8, 9, 64, 257 pairs with 25 % gross outliers (none for n <= 9) at 0 and 0.05 px of noise, threshold
0.1; one case of n = 1000 at 0.3 px, threshold 1.0.  SceauxCastle K, rotation 0.15 rad, baseline 1, points 4..9 deep.
Per case H = 200 sample sets are drawn with np.random.seed(s) through np.random.choice exactly as the reference's
generator draws them; each is run through the reference's estimate_fundamental_matrix_ransac alone (one iteration, the
sample replayed), which yields its F and its mask, and the best of them is checked against what the same function returns
for all H under the same seed.  Also recorded: estimate_fundamental_matrix over the inliers of the best hypothesis.
Pose cases: n = 8, 64, 257 outlier-free pairs at 0 and 0.3 px; E = K^T F K from the reference's n-point F; what its
recover_pose returns.

Bounds, by the rule of resect_bounds.json: the distance of the numpy restatement (tests/two_view_ref.py) to the
reference, the worst over the cases, times 100 -- for unit-norm sign-fixed F per hypothesis and refit, for R as an angle,
for t.

The generator asserts the conditions under which the reference alone passes the tests:
  * no recorded distance lies within 1e-6 x threshold of the threshold, and the restatement's masks equal the reference's,
    so masks and counts must be EXACTLY equal;
  * in every pose case the winner (the restatement's four counts, its mask equal to the one the reference's recover_pose
    returns) has strictly more pairs in front than any other candidate, and every depth of the winner is at least 1e-3
    away from 0.
It also times the reference's RANSAC on one edge of 2000 pairs at H = 1000 (tools/two_view_timing.py prints it beside the
device's time).

    python tools/gen_two_view_golden.py --reference /path/to/reference
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
for p in (ROOT, os.path.join(ROOT, "sfm-python_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

H = 200
FACTOR = 100.0
RANSAC_CASES = [(n, noise, 0.0 if n <= 9 else 0.25, 0.1) for n in (8, 9, 64, 257) for noise in (0.0, 0.05)] + [(1000, 0.3, 0.25, 1.0)]
POSE_CASES = [(n, noise) for n in (8, 64, 257) for noise in (0.0, 0.3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("SFM_REFERENCE", ""), help="checkout of the reference project")
    a = ap.parse_args()
    if not a.reference or not os.path.exists(os.path.join(a.reference, "cv2_lite", "recover_pose.py")):
        sys.exit("reference not present: fixtures can only be generated where its checkout is")
    sys.path.insert(0, a.reference)
    from cv2_lite import fundamental_matrix_estimation as fme     # the reference's own modules, by path
    from cv2_lite import recover_pose as rp
    import two_view_ref as tv
    from sfmba.synthetic import K_SCEAUX

    K = K_SCEAUX.copy()
    rng = np.random.default_rng(20240918)
    out = dict(K=K)
    meas = dict(F_hyp=[], F_refit=[], R_angle=[], t_dist=[])
    scored = flipped = 0
    min_gap = np.inf

    # ---- RANSAC ----
    p1s, p2s, ptr, samples = [], [], [0], []
    rec = dict(n=[], noise=[], threshold=[], seed=[], hyp_F=[], hyp_masks=[], hyp_inliers=[], best=[], inliers=[],
               success=[], F=[], F_refit=[], mask=[])
    for k, (n, noise, outl, thr) in enumerate(RANSAC_CASES):
        p1, p2, _, _, _ = tv.make_pairs(rng, n, K, noise=noise, outliers=outl)
        seed = 1000 + k
        np.random.seed(seed)
        smp = np.array([np.random.choice(n, 8, replace=False) for _ in range(H)], dtype=np.int32)
        # every recorded sample through the reference's own RANSAC: one iteration each, np.random.choice replaying the sample
        Fs, masks = np.empty((H, 3, 3)), np.empty((H, n), dtype=bool)
        real_choice = np.random.choice
        try:
            for h in range(H):
                np.random.choice = lambda *args, _idx=smp[h], **kw: _idx.copy()
                Fs[h], masks[h], _ = fme.estimate_fundamental_matrix_ransac(p1, p2, threshold=thr, maxIters=1)
        finally:
            np.random.choice = real_choice
        for h in range(H):                                       # how near the threshold a distance comes (the project's formula)
            dist = tv.distances(Fs[h], p1, p2)
            assert np.isfinite(dist).all() and np.array_equal(dist < thr, masks[h]), (n, noise, h)
            min_gap = min(min_gap, float(np.abs(dist - thr).min()) / thr)
        counts = masks.sum(axis=1)
        best = int(np.argmax(counts))                            # (the first of equal counts, as Python's max)
        np.random.seed(seed)
        F_run, mask_run, success = fme.estimate_fundamental_matrix_ransac(p1, p2, threshold=thr, maxIters=H)
        assert np.array_equal(F_run, Fs[best]) and np.array_equal(mask_run, masks[best]), (n, noise)
        # (a best hypothesis of fewer than 8 inliers -- eight noisy pairs after the rank-2 step -- has no refit: its own F)
        F_refit = fme.estimate_fundamental_matrix(p1[masks[best]], p2[masks[best]]) if counts[best] >= 8 else Fs[best]
        # the restatement on the same input
        mine = tv.ransac_edge(p1, p2, smp, threshold=thr, refit=True, margin=1e-6 * thr)
        assert mine["status"] == (tv.OK if counts[best] >= 8 else tv.DEGENERATE), (n, noise)
        assert mine["best"] == best and not mine["near"].any(), (n, noise)
        for h in range(H):
            m = tv.inliers(mine["hyp_F"][h], p1, p2, thr)
            flipped += int((m != masks[h]).sum())
            scored += n
            meas["F_hyp"].append(float(np.abs(tv.unit_F(mine["hyp_F"][h]) - tv.unit_F(Fs[h])).max()))
        assert np.array_equal(mine["hyp"], counts) and np.array_equal(mine["mask"], masks[best]), (n, noise)
        if counts[best] >= 8:
            meas["F_refit"].append(float(np.abs(mine["F_refit"] - tv.unit_F(F_refit)).max()))
        p1s.append(p1); p2s.append(p2); ptr.append(ptr[-1] + n); samples.append(smp)
        for key, val in (("n", n), ("noise", noise), ("threshold", thr), ("seed", seed), ("hyp_F", Fs),
                         ("hyp_masks", np.packbits(masks, axis=None)), ("hyp_inliers", counts.astype(np.int32)), ("best", best),
                         ("inliers", int(counts[best])), ("success", bool(success)), ("F", tv.unit_F(Fs[best])),
                         ("F_refit", tv.unit_F(F_refit)), ("mask", masks[best])):
            rec[key].append(val)
        print(f"ransac n={n:4d} noise={noise:.2f} thr={thr}: best h={best} with {counts[best]} inliers, success={bool(success)}; "
              f"restatement F within {max(meas['F_hyp'][-H:]):.2e}")
    assert flipped == 0 and min_gap > 1e-6, (flipped, min_gap)
    print(f"{scored} scored pairs, {flipped} flipped masks, nearest distance {min_gap:.2e} x threshold away from it")
    out.update(r_pts1=np.concatenate(p1s), r_pts2=np.concatenate(p2s), r_ptr=np.asarray(ptr, dtype=np.int64),
               r_samples=np.stack(samples), r_n=np.asarray(rec["n"], dtype=np.int64), r_noise=np.asarray(rec["noise"]),
               r_threshold=np.asarray(rec["threshold"]), r_seed=np.asarray(rec["seed"], dtype=np.int64),
               r_hyp_F=np.stack(rec["hyp_F"]), r_hyp_masks=np.concatenate(rec["hyp_masks"]),
               r_hyp_inliers=np.stack(rec["hyp_inliers"]), r_best=np.asarray(rec["best"], dtype=np.int32),
               r_inliers=np.asarray(rec["inliers"], dtype=np.int32), r_success=np.asarray(rec["success"]),
               r_F=np.stack(rec["F"]), r_F_refit=np.stack(rec["F_refit"]), r_mask=np.concatenate(rec["mask"]))

    # ---- pose ----
    p1s, p2s, ptr = [], [], [0]
    rec = dict(n=[], noise=[], E=[], R=[], t=[], mask=[], err=[], R_true=[], t_true=[])
    for n, noise in POSE_CASES:
        p1, p2, R_true, t_true, _ = tv.make_pairs(rng, n, K, noise=noise)
        F = fme.estimate_fundamental_matrix(p1, p2)
        E = K.T @ F @ K
        err, R, T, mask255 = rp.recover_pose(E, p1, p2, K)
        T, mask = np.asarray(T).ravel(), np.asarray(mask255).ravel() != 0
        # the four candidates' counts from the restatement, held against the reference's winner: the same mask, the winner
        # strictly ahead, its depths away from zero
        mine = tv.recover_pose_edge(E, p1, p2, K)
        counts = [int(c) for c in mine["front_all"]]
        win = int(np.argmax(counts))
        assert mine["status"] == tv.OK and np.array_equal(mine["mask"], mask) and counts[win] == mask.sum(), (n, noise, counts)
        assert counts[win] > max(c for i, c in enumerate(counts) if i != win), (n, noise, counts)
        depths = np.concatenate([mine["X"][:, 2], (mine["X"] @ mine["R"].T + mine["t"])[:, 2]])
        assert np.abs(depths).min() >= 1e-3, (n, noise, np.abs(depths).min())
        meas["R_angle"].append(tv.rotation_angle(R, mine["R"]))
        meas["t_dist"].append(float(np.linalg.norm(T - mine["t"])))
        p1s.append(p1); p2s.append(p2); ptr.append(ptr[-1] + n)
        for key, val in (("n", n), ("noise", noise), ("E", E), ("R", R), ("t", T), ("mask", mask), ("err", float(err)),
                         ("R_true", R_true), ("t_true", t_true)):
            rec[key].append(val)
        print(f"pose n={n:4d} noise={noise:.1f}: front {counts} (winner {win}); restatement R within {meas['R_angle'][-1]:.2e} rad, "
              f"t within {meas['t_dist'][-1]:.2e}")
    out.update(p_pts1=np.concatenate(p1s), p_pts2=np.concatenate(p2s), p_ptr=np.asarray(ptr, dtype=np.int64),
               p_n=np.asarray(rec["n"], dtype=np.int64), p_noise=np.asarray(rec["noise"]), p_E=np.stack(rec["E"]),
               p_R=np.stack(rec["R"]), p_t=np.stack(rec["t"]), p_mask=np.concatenate(rec["mask"]), p_err=np.asarray(rec["err"]),
               p_R_true=np.stack(rec["R_true"]), p_t_true=np.stack(rec["t_true"]))
    np.savez_compressed(os.path.join(OUT, "two_view_cases.npz"), **out)

    # ---- the reference's time for one edge of 2000 pairs at H = 1000 ----
    p1, p2, _, _, _ = tv.make_pairs(rng, 2000, K, noise=0.3, outliers=0.25)
    np.random.seed(7)
    t0 = time.perf_counter()
    fme.estimate_fundamental_matrix_ransac(p1, p2, threshold=1.0, maxIters=1000)
    ref_seconds = time.perf_counter() - t0
    print(f"reference RANSAC, 1 edge x 2000 pairs, H = 1000: {ref_seconds:.3f} s on this CPU")

    bounds = dict(factor=FACTOR, hypotheses=H, ransac_cases=[[int(n), float(z), float(t)] for n, z, _, t in RANSAC_CASES],
                  pose_cases=[[int(n), float(z)] for n, z in POSE_CASES], scored_pairs=int(scored), flipped_masks=int(flipped),
                  nearest_distance_over_threshold=float(min_gap), reference_cpu_seconds_1x2000_H1000=float(ref_seconds))
    for key in ("F_hyp", "F_refit", "R_angle", "t_dist"):
        bounds[key] = dict(measured_max=max(meas[key]), bound=FACTOR * max(meas[key]))
    with open(os.path.join(OUT, "two_view_bounds.json"), "w") as f:
        json.dump(bounds, f, indent=1)
        f.write("\n")
    print("wrote two_view_cases.npz, two_view_bounds.json")


if __name__ == "__main__":
    main()
