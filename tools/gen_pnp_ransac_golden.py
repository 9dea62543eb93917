#!/usr/bin/env python
"""Fixtures of the robust-resection tests: tests/golden/pnp_ransac_cases.npz and tests/golden/pnp_ransac_bounds.json.

Runs only where the reference checkout exists (never on the GPU box): its teaching implementation of cv2.solvePnP,
cv2_lite/solve_pnp.py, is imported from the checkout given with --reference and run on the INLIER SET that the numpy
restatement (tests/pnp_ransac_ref.py) finds -- the oracle of resect_bounds.json.  (The reference's cv2_lite/solve_p3p.py is
no oracle for the minimal solver: on exact data it returns no solution three times out of four and wrong ones
otherwise; the minimal solver is pinned by its own properties and by the generating pose.)  Outputs are data only.

Scenes: n = 8, 12, 64, 257 correspondences, SceauxCastle K, 0.5 px of pixel noise, 25-40 % of the pixels displaced by
20-200 px, all depths above 1, recorded samples, H = 64 hypotheses (256 at n = 257), threshold 2 px, min_views 4.

The generator asserts, so that the fixture cannot hide a failure:
  * the restatement's best mask holds NO displaced observation and at least 80 % of the others;
  * the best hypothesis is not `close`, and at most 2 % of a scene's hypotheses are;
  * the reference's solve_pnp on the restatement's inlier set reports success, and its final cost is not above the
    restatement's beyond rounding.

Bounds (the rule of resect_bounds.json: what the restatement itself is off by, times 100):
  final_R_angle, final_T_dist   the restatement's refined pose against the reference's recorded pose, worst scene
  p3p_R_angle, p3p_T_dist       the restatement's nearest P3P solution against the generating pose on the exact samples of
                                pnp_ransac_ref.exact_samples that are not `close`, worst sample
  p3p_reproj_px                 the largest reprojection error of a solution at its own three points, same samples

    python tools/gen_pnp_ransac_golden.py --reference /path/to/reference
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
for p in (ROOT, os.path.join(ROOT, "sfm-python_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

SIZES = (8, 12, 64, 257)
FACTOR = 100.0
THRESHOLD, MIN_VIEWS = 2.0, 4
EXACT_SEED, EXACT_COUNT = 20241019, 4000
SEED = 20241019


def hypotheses(n):
    return 256 if n >= 257 else 64


def make_scene(rng, n, K):
    """A random pose, n points 4..9 units in front of it, 0.5 px of noise, 25-40 % of the pixels displaced by 20-200 px."""
    import resect_ref as rr
    w = rng.normal(size=3)
    w *= rng.uniform(0.2, 1.0) / np.linalg.norm(w)
    R = rr.orc.rodrigues(w)
    T = rng.normal(0.0, 1.5, 3)
    cam = np.stack([rng.uniform(-1.8, 1.8, n), rng.uniform(-1.3, 1.3, n), rng.uniform(4.0, 9.0, n)], axis=1)
    X = cam @ R + T
    uv = cam @ K.T
    uv = uv[:, :2] / uv[:, 2:3] + 0.5 * rng.normal(size=(n, 2))
    n_bad = int(round(rng.uniform(0.25, 0.40) * n))
    bad = np.zeros(n, dtype=bool)
    bad[rng.choice(n, n_bad, replace=False)] = True
    ang = rng.uniform(0.0, 2.0 * np.pi, n)
    uv[bad] += (rng.uniform(20.0, 200.0, n)[:, None] * np.stack([np.cos(ang), np.sin(ang)], axis=1))[bad]
    return X, uv, bad, w, T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("SFM_REFERENCE", ""), help="checkout of the reference project")
    a = ap.parse_args()
    if not a.reference or not os.path.exists(os.path.join(a.reference, "cv2_lite", "solve_pnp.py")):
        sys.exit("reference not present: fixtures can only be generated where its checkout is")
    sys.path.insert(0, a.reference)
    from cv2_lite import solve_pnp as ref                        # the reference's own module, by path
    import pnp_ransac_ref as pr
    import resect_ref as rr
    from sfmba.synthetic import K_SCEAUX

    K = K_SCEAUX.copy()

    def scenes(seed):
        rng = np.random.default_rng(seed)
        Xs, uvs, bads, smp, ptr, hptr = [], [], [], [], [0], [0]
        rec = dict(n=[], H=[], rvec_true=[], T_true=[], rvec=[], tvec=[], inliers=[], best=[], best_sol=[], close_share=[])
        meas = dict(final_R_angle=[], final_T_dist=[], cost_ratio=[])
        for n in SIZES:
            H = hypotheses(n)
            X, uv, bad, w, T = make_scene(rng, n, K)
            samples = np.stack([rng.choice(n, 3, replace=False) for _ in range(H)]).astype(np.int32)
            r = pr.ransac_one(X, uv, K, samples=samples, max_iters=H, threshold=THRESHOLD, min_views=MIN_VIEWS)
            assert r["status"] == pr.OK, (n, r["status"])
            mask = r["mask"]
            assert not np.any(mask & bad), (n, "a displaced observation is in the best mask")
            assert mask.sum() >= 0.8 * (~bad).sum(), (n, int(mask.sum()), int((~bad).sum()))
            assert not r["hyp_close"][r["best"]], (n, "the best hypothesis is close")
            share = float(r["hyp_close"].mean())
            assert share <= 0.02, (n, share)
            success, rvec, tvec = ref.solve_pnp(X[mask], uv[mask], K)
            assert success, n
            rvec, tvec = np.asarray(rvec).ravel(), np.asarray(tvec).ravel()
            R_ref = rr.orc.rodrigues(rvec)
            p_ref = np.concatenate([rvec, -R_ref.T @ tvec])
            c_ref, c_mine = rr.cost(p_ref, X[mask], uv[mask], K), rr.cost(r["params"], X[mask], uv[mask], K)
            assert c_ref <= c_mine * (1.0 + 1e-9) + n * 1e-24, (n, c_ref, c_mine)      # (the rounding argument of gen_resect_golden.py)
            R_mine, _ = rr.pose_from_params(r["params"])
            meas["final_R_angle"].append(rr.rotation_angle(R_ref, R_mine))
            meas["final_T_dist"].append(float(np.linalg.norm(p_ref[3:] - r["params"][3:])))
            meas["cost_ratio"].append(float(c_ref / c_mine))
            Xs.append(X); uvs.append(uv); bads.append(bad); smp.append(samples)
            ptr.append(ptr[-1] + n); hptr.append(hptr[-1] + H)
            for key, val in (("n", n), ("H", H), ("rvec_true", w), ("T_true", T), ("rvec", rvec), ("tvec", tvec),
                             ("inliers", int(mask.sum())), ("best", int(r["best"])), ("best_sol", int(r["best_sol"])),
                             ("close_share", share)):
                rec[key].append(val)
            print(f"n={n:4d} H={H}: {int(bad.sum())} displaced, best h={r['best']} sol={r['best_sol']} with {int(mask.sum())} of "
                  f"{int((~bad).sum())} true inliers, close {100 * share:.2f} %, final R {meas['final_R_angle'][-1]:.2e} rad, "
                  f"T {meas['final_T_dist'][-1]:.2e}, {r['iters']} trial poses, rms {r['rms_err']:.3f} px")
        return Xs, uvs, bads, smp, ptr, hptr, rec, meas

    # the first seed from SEED on whose four scenes pass the assertions above (a scene of 64 hypotheses passes the 2 % test
    # with at most ONE close hypothesis, and about one hypothesis in a hundred is close)
    for seed in range(SEED, SEED + 50):
        try:
            Xs, uvs, bads, smp, ptr, hptr, rec, meas = scenes(seed)
            break
        except AssertionError as err:
            print(f"seed {seed}: {err}")
    else:
        sys.exit("no seed passed")
    print(f"scenes of seed {seed}")
    # the minimal solver on exact samples
    p3p = dict(R_angle=0.0, T_dist=0.0, reproj_px=0.0, close=0, found=0, above_1e6=0)
    dist = []
    for X, uv, w, T in pr.exact_samples(EXACT_SEED, EXACT_COUNT, K):
        sols, close = pr.p3p(X, uv, K)
        assert len(sols) <= 4
        R = rr.orc.rodrigues(w)
        d = [(rr.rotation_angle(R, S[0]), float(np.linalg.norm(S[1] - T))) for S in sols]
        assert d, "the generating pose is among the solutions"
        k = int(np.argmin([max(x) for x in d]))
        dist.append(max(d[k]))
        p3p["close"] += int(close)
        if close:
            continue
        p3p["R_angle"], p3p["T_dist"] = max(p3p["R_angle"], d[k][0]), max(p3p["T_dist"], d[k][1])
        for S in sols:
            p3p["reproj_px"] = max(p3p["reproj_px"], float(np.sqrt(pr.errors2(S[0], S[1], X, uv, K)[0].max())))
    dist = np.array(dist)
    print(f"P3P on {EXACT_COUNT} exact samples: nearest solution median {np.median(dist):.2e}, above 1e-6 in "
          f"{100 * (dist > 1e-6).mean():.2f} %, close {100 * p3p['close'] / EXACT_COUNT:.2f} %; not close: R {p3p['R_angle']:.2e} rad, "
          f"T {p3p['T_dist']:.2e}, own points {p3p['reproj_px']:.2e} px")
    np.savez_compressed(os.path.join(OUT, "pnp_ransac_cases.npz"), K=K, X=np.concatenate(Xs), uv=np.concatenate(uvs),
                        displaced=np.concatenate(bads), ptr=np.asarray(ptr, dtype=np.int64),
                        samples=np.concatenate(smp), hptr=np.asarray(hptr, dtype=np.int64),
                        n=np.asarray(rec["n"], dtype=np.int64), H=np.asarray(rec["H"], dtype=np.int64),
                        rvec_true=np.asarray(rec["rvec_true"]), T_true=np.asarray(rec["T_true"]),
                        rvec=np.asarray(rec["rvec"]), tvec=np.asarray(rec["tvec"]),
                        inliers=np.asarray(rec["inliers"], dtype=np.int64), best=np.asarray(rec["best"], dtype=np.int64),
                        best_sol=np.asarray(rec["best_sol"], dtype=np.int64),
                        threshold=np.float64(THRESHOLD), min_views=np.int64(MIN_VIEWS))
    bounds = dict(factor=FACTOR, close=pr.CLOSE, scene_seed=seed, cases=[int(n) for n in rec["n"]], close_share=rec["close_share"],
                  exact=dict(seed=EXACT_SEED, count=EXACT_COUNT, close=p3p["close"], median_distance=float(np.median(dist)),
                             share_above_1e6=float((dist > 1e-6).mean())))
    for key in ("final_R_angle", "final_T_dist"):
        bounds[key] = dict(measured=meas[key], measured_max=max(meas[key]), bound=FACTOR * max(meas[key]))
    for key in ("R_angle", "T_dist", "reproj_px"):
        bounds["p3p_" + key] = dict(measured_max=p3p[key], bound=FACTOR * p3p[key])
    bounds["cost_ratio_reference_over_restatement"] = meas["cost_ratio"]
    with open(os.path.join(OUT, "pnp_ransac_bounds.json"), "w") as f:
        json.dump(bounds, f, indent=1)
        f.write("\n")
    print("wrote pnp_ransac_cases.npz, pnp_ransac_bounds.json")


if __name__ == "__main__":
    main()
