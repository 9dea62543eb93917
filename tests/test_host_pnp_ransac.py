"""Host tests of the robust resection (sfmba_resect_ransac): the numpy restatement's P3P on exact samples, its closed-form
quartic roots against np.roots, the draw rule, the restatement against the fixture of tools/gen_pnp_ransac_golden.py, and
the argument checks of solve_pnp_ransac that need no device.

Bounds: tests/golden/pnp_ransac_bounds.json, every one the restatement's own distance (to the generating pose, to the
reference's recorded pose) times 100."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

import pnp_ransac_ref as pr
import resect_ref as rr

BOUNDS = json.load(open(os.path.join(GOLDEN, "pnp_ransac_bounds.json")))
K = np.array([[2905.88, 0.0, 1416.0], [0.0, 2905.88, 1064.0], [0.0, 0.0, 1.0]])


def fixture_scenes():
    g = np.load(os.path.join(GOLDEN, "pnp_ransac_cases.npz"), allow_pickle=False)
    for k in range(len(g["n"])):
        sl = slice(int(g["ptr"][k]), int(g["ptr"][k + 1]))
        hs = slice(int(g["hptr"][k]), int(g["hptr"][k + 1]))
        yield dict(k=k, n=int(g["n"][k]), H=int(g["H"][k]), X=g["X"][sl], uv=g["uv"][sl], displaced=g["displaced"][sl],
                   samples=g["samples"][hs], K=g["K"], threshold=float(g["threshold"]), min_views=int(g["min_views"]),
                   rvec=g["rvec"][k], tvec=g["tvec"][k], rvec_true=g["rvec_true"][k], T_true=g["T_true"][k],
                   inliers=int(g["inliers"][k]), best=int(g["best"][k]), best_sol=int(g["best_sol"][k]))


def test_p3p_on_exact_samples():
    ex = BOUNDS["exact"]
    n_close = 0
    worst = dict(R=0.0, T=0.0, px=0.0)
    for X, uv, w, T in pr.exact_samples(ex["seed"], 3000, K):
        sols, close = pr.p3p(X, uv, K)
        assert 1 <= len(sols) <= 4
        R = rr.orc.rodrigues(w)
        d = [(rr.rotation_angle(R, S[0]), float(np.linalg.norm(S[1] - T))) for S in sols]
        a, t = min(d, key=max)
        n_close += close
        if close:
            # the generating pose is still among the solutions, only less sharply (a double root halves the digits)
            assert a <= 1e-3 and t <= 1e-2, (a, t)
            continue
        assert a <= BOUNDS["p3p_R_angle"]["bound"] and t <= BOUNDS["p3p_T_dist"]["bound"], (a, t)
        worst["R"], worst["T"] = max(worst["R"], a), max(worst["T"], t)
        for S in sols:
            px = float(np.sqrt(pr.errors2(S[0], S[1], X, uv, K)[0].max()))
            worst["px"] = max(worst["px"], px)
            assert px <= BOUNDS["p3p_reproj_px"]["bound"], px
            assert abs(np.linalg.det(S[0]) - 1.0) <= 1e-9 and np.abs(S[0] @ S[0].T - np.eye(3)).max() <= 1e-9
    print(f"3000 exact samples, {n_close} close; worst not close: R {worst['R']:.2e} rad, T {worst['T']:.2e}, own points {worst['px']:.2e} px")
    assert n_close <= 0.02 * 3000


def test_p3p_degenerate_triples_have_no_solution():
    rng = np.random.default_rng(3)
    X, uv, w, T = next(pr.exact_samples(5, 1, K))
    line = np.stack([X[0], X[0] + 0.4 * (X[1] - X[0]), X[1]])
    cam = (line - T) @ rr.orc.rodrigues(w).T @ K.T
    assert pr.p3p(line, cam[:, :2] / cam[:, 2:3], K)[0] == []
    assert pr.p3p(np.stack([X[0], X[0], X[2]]), np.stack([uv[0], uv[0], uv[2]]), K)[0] == []
    assert pr.p3p(np.stack([X[0], X[1], X[0]]), np.stack([uv[0], uv[1], uv[0]]), K)[0] == []
    assert pr.p3p(np.full((3, 3), np.nan), uv, K)[0] == []
    h = pr.hypothesis(rng.normal(size=(5, 3)), rng.normal(size=(5, 2)), K, [1, 1, 2], 2.0, 0.0)
    assert h["count"] == -1 and h["sol"] == -1


def test_closed_form_quartic_roots_against_numpy():
    rng = np.random.default_rng(11)
    checked = 0
    for _ in range(3000):
        kind = rng.integers(3)
        if kind == 0:                                            # four real roots
            A = np.poly(rng.uniform(-3.0, 3.0, 4))[::-1]
        elif kind == 1:                                          # two real roots and a complex pair
            re, im = rng.uniform(-2.0, 2.0), rng.uniform(0.1, 2.0)
            A = np.poly(np.concatenate([rng.uniform(-3.0, 3.0, 2), [re + 1j * im, re - 1j * im]])).real[::-1]
        else:                                                    # no real root
            z = rng.uniform(-2.0, 2.0, 2) + 1j * rng.uniform(0.1, 2.0, 2)
            A = np.poly(np.concatenate([z, z.conj()])).real[::-1]
        A = A * rng.uniform(0.5, 2.0) * rng.choice([-1.0, 1.0])
        roots, close = pr.quartic_real_roots(list(A))
        if close:
            continue
        checked += 1
        want = np.roots(A[::-1])
        want = np.sort(want[np.abs(want.imag) <= 1e-9 * (1.0 + np.abs(want.real))].real)
        assert len(roots) == len(want) == (4, 2, 0)[kind], (A, roots, want)
        assert np.allclose(roots, want, rtol=1e-9, atol=1e-9), (A, roots, want)
        assert list(roots) == sorted(roots)
    assert checked >= 2500


def test_draw_rule():
    seen = set()
    for n in (3, 4, 5, 64, 1000):
        for c in (0, 1, 7):
            for h in range(40):
                idx = pr.draw3(9, c, h, n)
                assert len(set(idx)) == 3 and all(0 <= k < n for k in idx)
                seen.add((n, c, tuple(idx)))
    # a function of (seed, camera index in the problem, h) alone: another camera, seed or h draws another sample
    a = pr.draw_samples(5, 2, 64, 300)
    assert np.array_equal(a, pr.draw_samples(5, 2, 64, 300))
    assert not np.array_equal(a, pr.draw_samples(6, 2, 64, 300)) and not np.array_equal(a, pr.draw_samples(5, 3, 64, 300))
    assert len({tuple(r) for r in a}) > 60
    # every position is drawn, first draws spread evenly (n = 4: each about a quarter of 4000)
    first = np.bincount([pr.draw3(1, 0, h, 4)[0] for h in range(4000)], minlength=4)
    assert first.min() > 900 and first.max() < 1100
    # selecting other cameras changes nothing for camera 1
    C, lens = 3, [20, 30, 25]
    rng = np.random.default_rng(2)
    ci = np.repeat(np.arange(C), lens)
    pi = np.arange(len(ci))
    X, uv, w, T = next(pr.exact_samples(8, 1, K))
    x = np.concatenate([np.zeros(6 * C), rng.normal(size=3 * len(ci)) + np.tile([0, 0, 6.0], len(ci))])
    args = (C, len(ci), ci, pi, rng.uniform(0, 2000, (len(ci), 2)), K)
    one = pr.resect_ransac(x, args, select=[0, 1, 0], max_iters=16, seed=4)
    every = pr.resect_ransac(x, args, max_iters=16, seed=4)
    assert np.array_equal(one["hyp_inliers"][1], every["hyp_inliers"][1]) and one["status"][0] == pr.NOT_SELECTED


def test_restatement_against_the_fixture():
    for sc in fixture_scenes():
        r = pr.ransac_one(sc["X"], sc["uv"], sc["K"], samples=sc["samples"], max_iters=sc["H"], threshold=sc["threshold"],
                          min_views=sc["min_views"])
        assert r["status"] == pr.OK and r["best"] == sc["best"] and r["best_sol"] == sc["best_sol"] and r["inliers"] == sc["inliers"]
        assert not np.any(r["mask"] & sc["displaced"]) and r["mask"].sum() >= 0.8 * (~sc["displaced"]).sum()
        assert not r["hyp_close"][r["best"]] and r["hyp_close"].mean() <= 0.02
        assert r["hyp_inliers"].max() == r["inliers"] and int(np.argmax(r["hyp_inliers"])) == r["best"]
        R_ref = rr.orc.rodrigues(sc["rvec"])
        a = rr.rotation_angle(R_ref, rr.orc.rodrigues(r["params"][:3]))
        d = float(np.linalg.norm(r["params"][3:] + R_ref.T @ sc["tvec"]))
        print(f"n={sc['n']}: restatement vs reference R {a:.2e} rad, T {d:.2e}")
        assert a <= BOUNDS["final_R_angle"]["measured_max"] * 1.001 and d <= BOUNDS["final_T_dist"]["measured_max"] * 1.001
        # plain resection over ALL observations is what the feature replaces: far from the truth, or a high error
        # (no depth test, so that the verdict is about the error alone)
        plain = rr.resect_one(sc["X"], sc["uv"], sc["K"], max_rms_px=2.0, min_depth=-np.inf)
        far = False
        if plain["status"] == rr.OK:
            R_true = rr.orc.rodrigues(sc["rvec_true"])
            far = (rr.rotation_angle(R_true, rr.orc.rodrigues(plain["params"][:3])) > 100.0 * BOUNDS["final_R_angle"]["bound"]
                   or np.linalg.norm(plain["params"][3:] - sc["T_true"]) > 100.0 * BOUNDS["final_T_dist"]["bound"])
        assert plain["status"] == rr.HIGH_ERROR or far


def test_solve_pnp_ransac_argument_checks():
    import sfmba
    X, uv = np.zeros((8, 3)), np.zeros((8, 2))
    with pytest.raises(ValueError):
        sfmba.solve_pnp_ransac(X, uv, K, dist=np.array([0.1, 0.0, 0.0, 0.0]))
    with pytest.raises(ValueError):
        sfmba.solve_pnp_ransac(X[:, :2], uv, K)
    with pytest.raises(ValueError):
        sfmba.solve_pnp_ransac(X, uv[:5], K)
    with pytest.raises(ValueError):
        sfmba.solve_pnp_ransac(X, uv, K[:2])
    with pytest.raises(ValueError):
        sfmba.solve_pnp_ransac(X, uv, K, iterationsCount=0)


def test_header_library_and_binding_agree():
    from sfmba import _capi
    for name in ("sfmba_default_pnp_ransac_options", "sfmba_resect_ransac"):
        assert name in _capi.SYMBOLS
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "sfmba.h")).read()
    body = header[header.index("typedef struct sfmba_pnp_ransac_options {"):header.index("} sfmba_pnp_ransac_options;")]
    import re
    fields = re.findall(r"^\s+(?:double|uint64_t|int32_t)\s+(\w+);", body, flags=re.M)
    assert fields == [f[0] for f in _capi.PnpRansacOptions._fields_]
