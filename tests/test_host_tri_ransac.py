"""Robust triangulation without a device: the numpy restatement of sfmba_triangulate_ransac (tests/tri_ransac_ref.py)
against independent routes -- numpy.linalg.svd of the pair's four rows, the reference's recorded two-view points --, the
pair numbering (in Python and, under the host sanitizers, csrc/tri_pairs.hpp itself), the drawn pairs against the
family's counter rule, the symbols and the option structure, and the figures of tests/golden/tri_ransac_bounds.json that
the GPU tests rely on."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import pnp_ransac_ref as pr
import tri_ransac_ref as trr
import triangulate_ref as tr

PKG = os.path.join(ROOT, "sfm-python_amd")
BOUNDS = json.load(open(os.path.join(GOLDEN, "tri_ransac_bounds.json")))


def test_pair_point_equals_the_svd_route_and_the_recorded_two_view_points():
    g = np.load(os.path.join(GOLDEN, "triangulate_cases.npz"), allow_pickle=False)
    rec = json.load(open(os.path.join(GOLDEN, "triangulate_bounds.json")))
    worst = 0.0
    for k in range(g["pts1"].shape[1]):
        w, X = trr.pair_point(g["M1"], g["M2"], g["pts1"][:, k], g["pts2"][:, k])
        Xs = trr.pair_point(g["M1"], g["M2"], g["pts1"][:, k], g["pts2"][:, k], solver="svd")[1]
        assert abs(np.sqrt(w @ w) - 1.0) < 1e-12
        worst = max(worst, float(np.abs(X - g["X_ref"][:3, k]).max()), float(np.abs(X - Xs).max()))
    assert worst <= rec["fixture"]["bound_abs"]                    # the bound the n-view restatement is held to there
    # on the scene of the GPU tests: every pair of a few tracks, against the SVD, within the recorded distance
    x, args, _, _ = trr.case_inputs("arc_h10")
    C, P, ci, pi, uv, K = args
    M = tr.projection_matrices(x, C, K)
    order, ptr = tr.stored_runs(pi, P)
    d = 0.0
    for p in range(0, P, 7):
        idx = order[ptr[p]:ptr[p + 1]]
        for a, b in trr.hypothesis_pairs(len(idx), p, 0, 10 ** 6):
            Xj = trr.pair_point(M[ci[idx[a]]], M[ci[idx[b]]], uv[idx[a]], uv[idx[b]])[1]
            Xs = trr.pair_point(M[ci[idx[a]]], M[ci[idx[b]]], uv[idx[a]], uv[idx[b]], solver="svd")[1]
            cams = x[:6 * C].reshape(C, 6)
            if tr.widest_angle_deg(Xs, cams[ci[idx[[a, b]]], 3:]) >= 1.0:
                d = max(d, float(np.abs(Xj - Xs).max() / max(1.0, np.abs(Xs).max())))
    assert 0.0 < d <= BOUNDS["cases"]["arc_h10"]["pair_bound_rel"]


def test_pair_numbering_round_trip():
    for n in range(2, 80):
        pairs = [(i, j) for i in range(n) for j in range(i + 1, n)]
        assert len(pairs) == trr.pair_count(n)
        assert [trr.pair_unrank(n, h) for h in range(len(pairs))] == pairs
        assert [trr.pair_rank(n, i, j) for i, j in pairs] == list(range(len(pairs)))
    for n in (2000, 46341, 65536, 65537, 92682):
        M = trr.pair_count(n)
        for h in (0, 1, M // 3, M // 2, 2 ** 31 - 1, 2 ** 31, M - 2, M - 1):
            if 0 <= h < M:
                i, j = trr.pair_unrank(n, h)
                assert 0 <= i < j < n and trr.pair_rank(n, i, j) == h
    assert trr.pair_count(0) == trr.pair_count(1) == 0
    # all pairs up to and including M = H, drawn above: n = 5 has the ten pairs of H = 10, n = 6 has fifteen
    assert trr.hypothesis_pairs(5, 3, 0, 10) == [(i, j) for i in range(5) for j in range(i + 1, 5)]
    assert trr.hypothesis_pairs(6, 3, 0, 10) == [trr.draw2(0, 3, h, 6) for h in range(10)]


def test_pair_numbering_header_under_sanitizers():
    run = subprocess.run(["make", "-C", PKG, "tri-check"], capture_output=True, text=True, timeout=900)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "tri_pairs_check: ok" in run.stdout


def test_drawn_pairs_are_the_counter_rule_with_two_draws():
    """draw2 is the first two draws of the rule pnp_ransac_ref.draw3 restates (the third draw does not change them)."""
    rng = np.random.default_rng(0)
    for _ in range(500):
        seed, p, h, n = int(rng.integers(0, 2 ** 63)), int(rng.integers(0, 10 ** 6)), int(rng.integers(0, 4096)), int(rng.integers(3, 200))
        a, b = trr.draw2(seed, p, h, n)
        assert [a, b] == pr.draw3(seed, p, h, n)[:2] and a != b and 0 <= a < n and 0 <= b < n
    assert sorted(trr.draw2(7, 0, 0, 2)) == [0, 1]
    firsts = {trr.draw2(1, 5, h, 12) for h in range(64)}
    assert len(firsts) > 30                                         # (repeats are allowed; the draws are not stuck)


def test_symbols_struct_layout_and_python_surface():
    import sfmba
    from sfmba import _capi
    header = open(os.path.join(ROOT, "include", "sfmba.h")).read()
    for name in ("sfmba_triangulate_ransac", "sfmba_default_tri_ransac_options"):
        assert name in header and name in _capi.SIGNATURES
    lib = ctypes.CDLL(_capi.LIB_PATH)
    assert hasattr(lib, "sfmba_triangulate_ransac")
    S = _capi.TriRansacOptions
    assert ctypes.sizeof(S) == 80 and sum(ctypes.sizeof(t) for _, t in S._fields_) == 80            # no implicit padding
    assert [(f, getattr(S, f).offset) for f, _ in S._fields_] == [
        ("threshold", 0), ("min_depth", 8), ("min_pair_angle_deg", 16), ("seed", 24), ("max_pairs", 32), ("min_views", 36),
        ("refine", 40), ("profile", 44), ("max_iter", 48), ("reserved", 52), ("xtol", 56), ("min_angle_deg", 64),
        ("max_error_px", 72)]
    o = S()
    lib.sfmba_default_tri_ransac_options.argtypes = [ctypes.POINTER(S)]
    lib.sfmba_default_tri_ransac_options.restype = None
    lib.sfmba_default_tri_ransac_options(ctypes.byref(o))
    got = {f: getattr(o, f) for f, _ in S._fields_}
    assert got == dict(threshold=4.0, min_depth=0.0, min_pair_angle_deg=1.0, seed=0, max_pairs=64, min_views=2, refine=1,
                       profile=0, max_iter=10, reserved=0, xtol=1e-10, min_angle_deg=1.0, max_error_px=np.inf)
    assert {k: v for k, v in got.items() if k in trr.DEFAULTS} == trr.DEFAULTS
    assert hasattr(sfmba.Backend, "triangulate_ransac") and callable(sfmba.triangulate_tracks_ransac)
    assert issubclass(sfmba.RobustTriangulation, sfmba.Triangulation) and sfmba.RobustTriangulation.NO_CONSENSUS == 6
    import inspect
    assert inspect.signature(sfmba.reconstruct).parameters["robust_triangulation"].default is False


def test_restatement_by_hand_on_a_clean_and_a_spoilt_track():
    """Four views of one point without noise: every pair gives the point and counts 4.  One observation displaced by 50 px:
    the three pairs that hold it count less than the three that do not, the first of those wins, the mask leaves it out."""
    x, args, _ = trr.arc_scene(n_tracks=1, seed=3, noise=0.0, contaminate=False, lengths=[4])
    ref = trr.triangulate_ransac(x, args)
    assert ref["status"][0] == trr.OK and ref["best"][0] == 0 and list(ref["hyp_inliers"][0, :7]) == [4] * 6 + [-1]
    assert ref["inlier_mask"].all() and not ref["hyp_close"].any()
    uv = args[4].copy()
    uv[1] += [30.0, -40.0]
    ref = trr.triangulate_ransac(x, args[:4] + (uv,) + args[5:])
    counts = ref["hyp_inliers"][0, :6]                              # pairs 01 02 03 12 13 23
    assert list(counts[[1, 2, 5]]) == [3, 3, 3] and counts[[0, 3, 4]].max() <= 2
    assert ref["best"][0] == 1 and list(ref["inlier_mask"]) == [True, False, True, True]
    assert ref["status"][0] == trr.OK and ref["inliers"][0] == 3 and ref["views"][0] == 4
    assert np.abs(ref["points"][0] - ref["hyp"][0]).max() < 1e-6
    # the same track under a tight error bound without the RANSAC: refused as a whole
    plain = tr.triangulate(x, args[:4] + (uv,) + args[5:], max_error_px=4.0)
    assert plain["status"][0] == tr.HIGH_ERROR


def test_bounds_file_is_what_the_restatement_gives():
    """The recorded figures of the smallest case are recomputed here; every case keeps its conditions: at most close_cap of
    the hypotheses close, at least nine contaminated tracks in ten recovered exactly."""
    assert BOUNDS["factor"] == 100.0 and BOUNDS["close_cap"] == 0.05 and BOUNDS["close_relative"] == trr.CLOSE
    assert set(BOUNDS["cases"]) == set(trr.CASES)
    for name, rec in BOUNDS["cases"].items():
        assert rec["close_share"] <= BOUNDS["close_cap"], name
        if name.startswith("arc"):                              # the contaminated scenes: the fixture must not degrade
            assert rec["recovered_share"] >= 0.9 and rec["contaminated_tracks"] >= 50, name
            assert rec["plain_ok"] == 0 and rec["plain_high_error"] + rec["plain_behind"] == rec["contaminated_tracks"], name
        assert rec["pair_bound_rel"] == 100.0 * rec["pair_measured_rel"] > 0.0
        assert rec["final_linear_bound_rel"] == 100.0 * rec["final_linear_measured_rel"] > 0.0
        assert rec["pair_bound_rel"] < 1e-6 and rec["final_linear_bound_rel"] < 1e-9       # (a bound that binds)
    now, _ = trr.measure_case("arc_h10")
    for key, value in now.items():
        assert BOUNDS["cases"]["arc_h10"][key] == pytest.approx(value, rel=1e-6, abs=0), key


def test_contaminated_tracks_fail_plainly_and_are_recovered_by_pairs():
    """What the feature is for, on the CPU: on the contaminated tracks of the scene the all-view DLT leaves an error above
    the threshold, the best pair's mask is the planted truth for at least nine in ten."""
    x, args, planted, options = trr.case_inputs("arc_h10")
    C, P, ci, pi, uv, K = args
    bad = np.flatnonzero(np.bincount(pi[planted], minlength=P) > 0)
    plain = tr.triangulate(x, args, max_error_px=4.0)
    # none comes back: HIGH_ERROR, or BEHIND where the bent point lies behind a camera (first match wins, BEHIND comes first)
    rec = BOUNDS["cases"]["arc_h10"]
    assert np.all(plain["status"][bad] != tr.OK)
    assert int((plain["status"][bad] == tr.HIGH_ERROR).sum()) == rec["plain_high_error"]
    assert int((plain["status"][bad] == tr.BEHIND).sum()) == rec["plain_behind"] == len(bad) - rec["plain_high_error"]
    assert len(bad) == rec["contaminated_tracks"] and rec["recovered"] >= 0.9 * len(bad)
