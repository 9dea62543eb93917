"""GPU tests of sfmba_triangulate_ransac (Backend.triangulate_ransac) against its numpy restatement
(tests/tri_ransac_ref.py): counts and bests, points, the edges of every loop and switch of k_tri_ransac, every status, the
masks, independence and repeatability, fp32 storage, isolation from the solver, the contaminated tracks the feature is
for, reconstruct(robust_triangulation=True) and the timing entry.

Counts are compared exactly wherever the restatement does not flag a hypothesis `close`; a point's best, mask, count and
status unless a close hypothesis could be its best or level with it (tri_ransac_ref.sure_points).  Points within
tests/golden/tri_ransac_bounds.json (tools/gen_tri_ransac_golden.py): 100 x the distance, measured on the CPU on the
tests' own inputs, between the Jacobi route and the SVD of the same rows.  Two refinements that both stop on xtol lie
within 200 xtol (|X| + xtol) of each other (test_gpu_triangulate.py).  The bounds are recorded per scene: "arc*" for the
contaminated 12-camera scenes, "edges*" for the 40-camera scene of the track-length switches with every option set run on
it.  The small scenes of the chunk, status and P = 1 tests come from the same generator and camera arc as "arc" with other
seeds and borrow its bounds: nothing was measured on them."""
import json
import os

import numpy as np
import pytest

import tri_ransac_ref as trr
import triangulate_ref as tr
from conftest import GOLDEN
from kernel_source import kernel_constant

pytestmark = pytest.mark.gpu

XTOL = 1e-10
BOUNDS = json.load(open(os.path.join(GOLDEN, "tri_ransac_bounds.json")))
L = kernel_constant("kStatsLongTrack")
WG = kernel_constant("kTriRansacThreads")                      # the workgroup's width = the points of a chunk
FIELDS = ("points", "hyp", "inlier_mask", "status", "views", "inliers", "best", "iters", "rms_err", "angle_deg")


@pytest.fixture(scope="module")
def be():
    import sfmba
    b = sfmba.Backend(0)
    yield b
    b.close()


def set_problem(be, args, bits=64):
    be.set_precision(bits)
    be.set_fixed_cameras(())
    be.set_problem(*args)


def rel(a, b):
    return float(np.abs(a - b).max() / max(1.0, np.abs(b).max()))


def check_against(res, ref, case, what="", refined=True):
    """Everything the restatement pins -> the number of points compared in full.  `case`: the case of
    tests/golden/tri_ransac_bounds.json whose recorded bounds hold."""
    rec = BOUNDS["cases"][case]
    assert np.array_equal(res.views, ref["views"]), what
    exists = ref["hyp_inliers"] >= 0
    if res.hyp_inliers is not None:
        assert np.array_equal(res.hyp_inliers >= 0, exists), what
        sure_h = ~ref["hyp_close"]
        assert np.array_equal(res.hyp_inliers[sure_h], ref["hyp_inliers"][sure_h]), what
    if exists.any():
        share = ref["hyp_close"].sum() / exists.sum()
        assert share <= BOUNDS["close_cap"], (what, share)
    sure = trr.sure_points(ref)
    worst_h = worst_x = 0.0
    for p in np.flatnonzero(sure):
        for key in ("status", "best", "inliers"):
            assert getattr(res, key)[p] == ref[key][p], (what, p, key, getattr(res, key)[p], ref[key][p])
        d = rel(res.hyp[p], ref["hyp"][p])
        worst_h = max(worst_h, d)
        assert d <= rec["pair_bound_rel"], (what, p, d)
        if ref["status"][p] == trr.OK:
            X = ref["points"][p]
            gap = float(np.sqrt(((res.points[p] - X) ** 2).sum()))
            lim = rec["final_linear_bound_rel"] * max(1.0, np.abs(X).max()) + (200.0 * XTOL * (np.sqrt(X @ X) + XTOL) if refined else 0.0)
            worst_x = max(worst_x, gap / lim)
            assert gap <= lim, (what, p, gap, lim)
        else:
            assert res.points[p].tobytes() == ref["points"][p].tobytes(), (what, p)       # the point of x
    of_sure = sure[ref["pi"]]                                    # observations of the points compared in full
    assert np.array_equal(res.inlier_mask[of_sure], ref["inlier_mask"][of_sure]), what
    print(f"{what}: {int(sure.sum())} of {len(sure)} points in full, {int(ref['hyp_close'].sum())} of {int(exists.sum())} "
          f"hypotheses close; X_hyp vs restatement {worst_h:.2e} (bound {rec['pair_bound_rel']:.2e}), X_out at {worst_x:.2f} of its bound")
    assert res.n_ok == int((res.status == res.OK).sum())
    return int(sure.sum())


def reference(x, args, **kw):
    ref = trr.triangulate_ransac(x, args, **kw)
    ref["pi"] = np.asarray(args[3]).ravel()
    return ref


@pytest.fixture(scope="module")
def cases():
    """The restatement on the scenes of tri_ransac_ref.CASES, computed once."""
    out = {}
    for name in trr.CASES:
        x, args, planted, options = trr.case_inputs(name)
        out[name] = (x, args, planted, options, reference(x, args, **options))
    return out


# ---- tests 1, 2, 7: counts, bests and points on the contaminated scene, fp64 and fp32 storage ------------------------------

@pytest.mark.parametrize("name", list(trr.CASES))
def test_counts_bests_and_points(be, cases, name):
    x, args, planted, options, ref = cases[name]
    bits = 32 if trr.CASES[name]["f32"] else 64
    rec = BOUNDS["cases"][name]
    try:
        set_problem(be, args, bits)
        res = be.triangulate_ransac(x, want_hyp=True, **options)
        lin = be.triangulate_ransac(x, refine=0, **options)
    finally:
        be.set_precision(64)
    exists = ref["hyp_inliers"] >= 0
    assert int(exists.sum()) == rec["hypotheses"] and int(ref["hyp_close"].sum()) == rec["close"]     # the recorded share is this one
    n = check_against(res, ref, name, name)
    assert n >= 0.9 * args[1] and n == rec["sure_points"]
    # refine = 0: the n-view DLT over the inliers, against the restatement's linear point
    worst = 0.0
    for p in np.flatnonzero(trr.sure_points(ref) & (ref["status"] == trr.OK)):
        worst = max(worst, rel(lin.points[p], ref["linear"][p]))
    print(f"{name}: refine = 0 vs the restatement's linear point {worst:.2e} (bound {rec['final_linear_bound_rel']:.2e})")
    assert worst <= rec["final_linear_bound_rel"] and np.all(lin.iters == 0)
    assert lin.inlier_mask.tobytes() == res.inlier_mask.tobytes() and lin.hyp.tobytes() == res.hyp.tobytes()
    if bits == 32:                                               # the rounded pixels were read, not the given ones
        C, P, ci, pi, uv, K = args
        given = trr.arc_scene(**trr.CASES[name]["scene"])[1][4]
        assert np.abs(given - uv).max() > 1e-6
        ok = np.flatnonzero(res.status == res.OK)[:40]
        order, ptr = tr.stored_runs(pi, P)
        cams = x[:6 * C].reshape(C, 6)
        for p in ok:
            idx = order[ptr[p]:ptr[p + 1]]
            idx = idx[res.inlier_mask[idx]]
            rms_r = np.sqrt(2.0 * tr.cost(res.points[p], cams, ci[idx], uv[idx], K) / len(idx))
            assert abs(res.rms_err[p] - rms_r) <= 1e-10 * max(rms_r, 1e-3), p


# ---- test 9: what the feature is for --------------------------------------------------------------------------------------------

def test_contaminated_tracks_keep_their_points(be, cases):
    x, args, planted, options, ref = cases["arc"]
    C, P, ci, pi, uv, K = args
    rec = BOUNDS["cases"]["arc"]
    bad = np.flatnonzero(np.bincount(pi[planted], minlength=P) > 0)
    assert len(bad) == rec["contaminated_tracks"] >= 150
    set_problem(be, args)
    plain = be.triangulate(x, max_error_px=4.0)
    # none comes back: HIGH_ERROR, or BEHIND where the bent point lies behind a camera (first match wins, and BEHIND comes
    # first) -- as many of each as the restatement of the plain call finds (recorded)
    assert np.all(plain.status[bad] != plain.OK) and rec["plain_ok"] == 0
    assert int((plain.status[bad] == plain.HIGH_ERROR).sum()) == rec["plain_high_error"]
    assert int((plain.status[bad] == plain.BEHIND).sum()) == rec["plain_behind"] == len(bad) - rec["plain_high_error"]
    res = be.triangulate_ransac(x, **options)
    order, ptr = tr.stored_runs(pi, P)
    sure = trr.sure_points(ref)

    def exact(r_status, r_mask, p):
        run = order[ptr[p]:ptr[p + 1]]
        return r_status[p] == trr.OK and np.array_equal(r_mask[run], ~planted[run])

    got = sum(exact(res.status, res.inlier_mask, p) for p in bad if sure[p])
    want = sum(exact(ref["status"], ref["inlier_mask"], p) for p in bad if sure[p])
    print(f"contaminated tracks: {len(bad)}, recovered exactly: device {got}, restatement {want} (recorded {rec['recovered']}), "
          f"left out as close {int((~sure[bad]).sum())}")
    assert got >= want and rec["recovered"] >= 0.9 * len(bad) and want >= rec["recovered"] - int((~sure[bad]).sum())
    assert not np.any(res.inlier_mask & planted & sure[pi] & (res.status == res.OK)[pi] & (ref["status"] == trr.OK)[pi] &
                      ~ref["inlier_mask"])


# ---- test 3: the edges of every loop and switch ---------------------------------------------------------------------------------

EDGE_LENGTHS = trr.edge_lengths()


@pytest.fixture(scope="module")
def edges():
    """40 cameras; the tracks of EDGE_LENGTHS between tracks of 2-4 views, 45 points (tri_ransac_ref.edge_scene)."""
    x, args, planted = trr.arc_scene(**trr.edge_scene())
    return x, args, {3 * k + 1: n for k, n in enumerate(EDGE_LENGTHS)}


@pytest.mark.parametrize("H", [64, 10, 1])
def test_track_lengths_at_the_switches(be, edges, H):
    """n = 2, 3, 4; M = H and M > H (H = 10: n = 5, 6; H = 64: n = 11, 12); the lane / wave switch at kStatsLongTrack - 1,
    itself, + 1; the wave form at one block, one block and one, two blocks and one; H = 1."""
    x, args, where = edges
    C, P, ci, pi, uv, K = args
    n_of = np.bincount(pi, minlength=P)
    opts = dict(max_pairs=H, seed=11)
    assert opts in trr.EDGE_OPTIONS                              # (its pairs are among those the bounds were measured on)
    ref = reference(x, args, **opts)
    set_problem(be, args)
    res = be.triangulate_ransac(x, want_hyp=True, **opts)
    assert check_against(res, ref, "edges", f"H={H}") >= P - 4
    for p, n in where.items():
        M = n * (n - 1) // 2
        assert n_of[p] == n and res.views[p] == n
        assert int((res.hyp_inliers[p] >= 0).sum()) == min(M, H)              # exhaustive up to and including M = H
        if M <= H:
            assert res.best[p] < M
    if H == 64:
        # n = 2: one hypothesis, and the result is sfmba_triangulate's
        two = np.flatnonzero(n_of == 2)
        plain = be.triangulate(x)
        assert np.array_equal(res.best[two], np.zeros(len(two), dtype=np.int32))
        both = two[res.inliers[two] == 2]
        assert len(both) >= len(two) - 2
        assert np.array_equal(res.status[both], plain.status[both]) and np.array_equal(res.views[both], plain.views[both])
        lim = BOUNDS["cases"]["edges"]["final_linear_bound_rel"]
        for p in both[res.status[both] == res.OK]:
            X = plain.points[p]
            assert np.sqrt(((res.points[p] - X) ** 2).sum()) <= lim * max(1.0, np.abs(X).max()) + 200.0 * XTOL * (np.sqrt(X @ X) + XTOL)


def chunk_problem(special):
    """WG + 1 tracks of two views, but for the tracks of `special` {point: views}; 12 cameras."""
    lens = np.full(WG + 1, 2)
    for p, n in special.items():
        lens[p] = n
    return trr.arc_scene(n_tracks=len(lens), seed=13, lengths=lens, contaminate=False)


def test_rounds_of_the_workgroup(be):
    """A chunk whose hypotheses number exactly the workgroup's width, one above it, one hypothesis in all; a point whose
    hypotheses straddle two rounds and two waves; P = 1; P one above the chunk size."""
    x, args, _ = chunk_problem({})
    C, P, ci, pi, uv, K = args
    assert P == WG + 1
    set_problem(be, args)
    full = be.triangulate_ransac(x, want_hyp=True)
    ref = reference(x, args)
    assert check_against(full, ref, "arc", "chunk of two-view tracks") >= P - 2
    assert int((full.hyp_inliers[:WG] >= 0).sum()) == WG                       # exactly one round for the first chunk
    one = np.zeros(P, dtype=bool)
    one[5] = True
    alone = be.triangulate_ransac(x, select=one, want_hyp=True)                  # one hypothesis in the whole launch
    for name in FIELDS:
        a, b = getattr(alone, name), getattr(full, name)
        assert a[pi == 5].tobytes() == b[pi == 5].tobytes() if name == "inlier_mask" else a[5].tobytes() == b[5].tobytes(), name
    assert np.all(alone.status[~one] == alone.NOT_SELECTED) and alone.n_ok == int(alone.status[5] == alone.OK)
    # WG + 2 hypotheses in the first chunk (one track of three views), then WG + 1 (one two-view track deselected)
    x3, args3, _ = chunk_problem({100: 3})
    set_problem(be, args3)
    ref3 = reference(x3, args3)
    assert int((ref3["hyp_inliers"][:WG] >= 0).sum()) == WG + 2
    assert check_against(be.triangulate_ransac(x3, want_hyp=True), ref3, "arc", "WG + 2") >= P - 2
    sel = np.ones(P, dtype=bool)
    sel[7] = False
    refs = reference(x3, args3, select=sel)
    assert int((refs["hyp_inliers"][:WG] >= 0).sum()) == WG + 1
    assert check_against(be.triangulate_ransac(x3, select=sel, want_hyp=True), refs, "arc", "WG + 1") >= P - 2
    # a twelve-view track (64 drawn hypotheses) behind 230 two-view tracks: numbers 230 .. 293 of the chunk, over the end of
    # the first round (256) and of a wave in each round
    xs, argss, _ = chunk_problem({230: 12})
    set_problem(be, argss)
    refs = reference(xs, argss)
    first = int((refs["hyp_inliers"][:230] >= 0).sum())
    assert first == 230 and first < WG < first + 64
    assert check_against(be.triangulate_ransac(xs, want_hyp=True), refs, "arc", "straddling") >= P - 2
    # P = 1
    x1, args1, _ = trr.arc_scene(n_tracks=1, seed=5, lengths=[7])
    set_problem(be, args1)
    assert check_against(be.triangulate_ransac(x1, want_hyp=True), reference(x1, args1), "arc", "P = 1") == 1


# ---- test 4: every status --------------------------------------------------------------------------------------------------------

def test_every_status(be):
    from sfmba import RobustTriangulation as R
    lens = [5, 5, 1, 5, 5, 5, 5, 5, 2]
    x, args, _ = trr.arc_scene(n_tracks=len(lens), seed=21, lengths=lens, contaminate=False, noise=0.2)
    C, P, ci, pi, uv, K = args
    uv = uv.copy()
    rng = np.random.default_rng(3)
    # 3: NO_CONSENSUS for want of inliers -- every observation moved by 30-60 px its own way; min_views = 4
    run = np.flatnonzero(pi == 3)
    uv[run] += rng.uniform(30.0, 60.0, (5, 2)) * rng.choice([-1.0, 1.0], (5, 2))
    # 4: NO_CONSENSUS for want of a valid pair -- all five observations by ONE camera (every pair's angle is zero)
    ci = ci.copy()
    ci[pi == 4] = ci[pi == 4][0]
    args = (C, P, ci, pi, uv, K)
    sel = np.ones(P, dtype=bool)
    sel[1] = False                                               # 1: not selected, between selected ones
    set_problem(be, args)
    opts = dict(min_views=4)
    res = be.triangulate_ransac(x, select=sel, want_hyp=True, **opts)
    ref = reference(x, args, select=sel, **opts)
    check_against(res, ref, "arc", "statuses")
    assert list(res.status[:5]) == [R.OK, R.NOT_SELECTED, R.FEW_VIEWS, R.NO_CONSENSUS, R.NO_CONSENSUS]
    assert res.status[8] == R.FEW_VIEWS and res.views[8] == 2 and res.best[8] == -1     # two views against min_views = 4
    # not selected: documented values, the point of x, no mask
    X0 = x[6 * C:].reshape(P, 3)
    assert res.views[1] == 0 and res.inliers[1] == 0 and res.best[1] == -1 and res.iters[1] == 0
    assert np.isnan(res.rms_err[1]) and np.isnan(res.angle_deg[1]) and not res.inlier_mask[pi == 1].any()
    assert res.points[1].tobytes() == X0[1].tobytes() and res.hyp[1].tobytes() == X0[1].tobytes()
    assert np.all(res.hyp_inliers[1] == -1) and np.all(res.hyp_inliers[2] == -1)
    assert res.views[2] == 1 and res.best[2] == -1
    # NO_CONSENSUS for want of inliers still reports hyp, count, h and mask
    assert 2 <= res.inliers[3] < 4 and res.best[3] >= 0 and res.inlier_mask[pi == 3].sum() == res.inliers[3]
    assert res.hyp[3].tobytes() != X0[3].tobytes() and res.points[3].tobytes() == X0[3].tobytes()
    assert np.isnan(res.rms_err[3]) and res.iters[3] == 0
    # ... for want of a valid pair: every count 0, the first hypothesis, the point of x, an empty mask
    assert np.all(res.hyp_inliers[4, :10] == 0) and res.best[4] == 0 and res.inliers[4] == 0
    assert res.hyp[4].tobytes() == X0[4].tobytes() and not res.inlier_mask[pi == 4].any()
    # k_triangulate's verdicts over the inliers: BEHIND, LOW_ANGLE and HIGH_ERROR by thresholds no clean track can pass
    assert np.all(be.triangulate_ransac(x, min_angle_deg=170.0).status[[0, 5, 6, 7]] == R.LOW_ANGLE)
    assert np.all(be.triangulate_ransac(x, max_error_px=1e-9).status[[0, 5, 6, 7]] == R.HIGH_ERROR)
    # a depth no point has: no pair is valid
    assert np.all(be.triangulate_ransac(x, min_depth=1e3).status[[0, 5, 6, 7]] == R.NO_CONSENSUS)
    for kw in (dict(min_angle_deg=170.0), dict(max_error_px=1e-9), dict(min_depth=1e3)):
        assert np.array_equal(be.triangulate_ransac(x, **kw).status, reference(x, args, **kw)["status"]), kw


@pytest.mark.parametrize("n", [4, 6])
def test_status_at_infinity_after_a_consensus(be, n):
    """AT_INFINITY is k_triangulate's verdict for anything non-finite.  threshold = +inf is no NaN and is accepted; two
    observations of a clean track are given finite pixels of magnitude 1.3e154, whose squared error, about 1.69e308, is
    finite and so below the threshold: the first pair, (0, 1), is valid and counts every observation, and in k_triangulate
    the sum of the squared errors over the inliers, twice that figure, overflows.  The restatement flags the best
    hypothesis close (it compares inf with inf), so the device's values are asserted directly."""
    x, args, _ = trr.arc_scene(n_tracks=1, seed=3, noise=0.2, contaminate=False, lengths=[n])
    C, P, ci, pi, uv, K = args
    uv = uv.copy()
    uv[2], uv[3] = [1.3e154, 0.0], [0.0, 1.3e154]
    args = (C, P, ci, pi, uv, K)
    x = x.copy()
    x[6 * C:] = [0.25, -0.5, 3.0]                                 # the point of x, to be handed back
    clean = reference(x, (C, P, ci[:2], pi[:2], uv[:2], K))        # the pair (0, 1) alone: its point
    assert clean["status"][0] == trr.OK and not clean["hyp_close"].any()
    set_problem(be, args)
    res = be.triangulate_ransac(x, threshold=np.inf, want_hyp=True)
    M = n * (n - 1) // 2
    assert res.status[0] == res.AT_INFINITY == 2 and res.n_ok == 0
    assert res.views[0] == n and res.best[0] == 0 and res.inliers[0] == n and res.inlier_mask.all()
    assert res.hyp_inliers[0, 0] == n and np.all(res.hyp_inliers[0, M:] == -1)
    assert np.all(res.hyp_inliers[0, :M] >= 0) and res.hyp_inliers[0].max() == n       # (h = 0 is the first of the largest)
    assert rel(res.hyp[0], clean["hyp"][0]) <= BOUNDS["cases"]["arc"]["pair_bound_rel"]       # X_hyp is reported
    assert res.points[0].tobytes() == x[6 * C:].tobytes()                                     # X_out: the point of x
    assert res.iters[0] == 0 and np.isnan(res.rms_err[0]) and np.isnan(res.angle_deg[0])


def test_status_behind_after_a_consensus(be, cases):
    """BEHIND needs an inlier that is in front of its camera at the pair's point and not at the refined one: min_depth is put
    between the two smallest depths of a track whose refined point lies nearer to a camera than its best pair's point."""
    x, args, planted, options, ref = cases["arc_h10"]
    C, P, ci, pi, uv, K = args
    cams = x[:6 * C].reshape(C, 6)
    Rc = tr.orc.rodrigues(cams[:, :3])
    order, ptr = tr.stored_runs(pi, P)
    set_problem(be, args)
    found = 0
    for p in np.flatnonzero(ref["status"] == trr.OK):
        idx = order[ptr[p]:ptr[p + 1]]
        idx = idx[ref["inlier_mask"][idx]]
        d_hyp = trr.project(ref["hyp"][p], Rc[ci[idx]], cams[ci[idx], 3:], K)[1].min()
        d_fin = trr.project(ref["points"][p], Rc[ci[idx]], cams[ci[idx], 3:], K)[1].min()
        if not d_fin < d_hyp - 1e-5:
            continue
        one = np.zeros(P, dtype=bool)
        one[p] = True
        kw = dict(options, min_depth=0.5 * (d_fin + d_hyp))
        want = reference(x, args, select=one, **kw)
        if want["status"][p] != trr.BEHIND or want["hyp_close"][p].any():
            continue
        res = be.triangulate_ransac(x, select=one, **kw)
        assert res.status[p] == res.BEHIND and res.best[p] == want["best"][p] and res.inliers[p] == want["inliers"][p]
        assert res.points[p].tobytes() == x[6 * C:].reshape(P, 3)[p].tobytes() and res.rms_err[p] > 0.0
        found += 1
        if found == 3:
            break
    assert found >= 1


# ---- test 5: masks ----------------------------------------------------------------------------------------------------------------

def test_masks(be, edges):
    x, args, where = edges
    C, P, ci, pi, uv, K = args
    rng = np.random.default_rng(4)
    use = rng.permutation(len(ci)) >= len(ci) // 6
    sel = rng.random(P) < 0.8
    opts = dict(max_pairs=20, seed=9)
    set_problem(be, args)
    masked = be.triangulate_ransac(x, obs_use=use, select=sel, want_hyp=True, **opts)
    set_problem(be, (C, P, ci[use], pi[use], uv[use], K))          # the problem without them (the points keep their numbers)
    removed = be.triangulate_ransac(x, select=sel, want_hyp=True, **opts)
    n_st, n_rm = np.bincount(pi, minlength=P), np.bincount(pi[use], minlength=P)
    # k_triangulate, unchanged, adds a run of fewer than kStatsLongTrack STORED observations in stored order: the same sums
    # in both problems; a longer run goes lane by lane of the wave from its stored positions, which the mask shifts
    same_form = (n_st < L) & (n_rm < L)
    assert (~same_form).sum() >= 5 and same_form.sum() >= P - 6
    for name in ("hyp", "status", "views", "inliers", "best", "hyp_inliers"):
        assert getattr(masked, name).tobytes() == getattr(removed, name).tobytes(), name
    assert np.array_equal(masked.inlier_mask[use], removed.inlier_mask) and not masked.inlier_mask[~use].any()
    for name in ("points", "iters", "rms_err", "angle_deg"):
        assert getattr(masked, name)[same_form].tobytes() == getattr(removed, name)[same_form].tobytes(), name
    for p in np.flatnonzero(~same_form & (masked.status == masked.OK)):
        X = removed.points[p]
        assert np.sqrt(((masked.points[p] - X) ** 2).sum()) <= 200.0 * XTOL * (np.sqrt(X @ X) + XTOL)
    # unselected rows at their documented values
    X0 = x[6 * C:].reshape(P, 3)
    off = ~sel
    assert np.all(masked.status[off] == -1) and not masked.views[off].any() and not masked.inliers[off].any()
    assert np.all(masked.best[off] == -1) and np.all(masked.hyp_inliers[off] == -1) and not masked.inlier_mask[off[pi]].any()
    assert masked.points[off].tobytes() == X0[off].tobytes() and masked.hyp[off].tobytes() == X0[off].tobytes()
    assert np.isnan(masked.rms_err[off]).all() and np.isnan(masked.angle_deg[off]).all() and not masked.iters[off].any()


# ---- test 6: independence and repeatability -------------------------------------------------------------------------------------

def test_same_bits_alone_twice_and_shuffled(be, edges):
    x, args, where = edges
    C, P, ci, pi, uv, K = args
    opts = dict(max_pairs=10000, seed=2)                         # every pair of every track: no draw depends on a point's index
    set_problem(be, args)
    first, again = be.triangulate_ransac(x, want_hyp=True, **opts), be.triangulate_ransac(x, want_hyp=True, **opts)
    for name in FIELDS + ("hyp_inliers",):
        assert getattr(first, name).tobytes() == getattr(again, name).tobytes(), name
    assert int((first.hyp_inliers[3 * EDGE_LENGTHS.index(129) + 1] >= 0).sum()) == 129 * 128 // 2
    for p in list(where) + [0, P - 1]:                           # each alone
        one = np.zeros(P, dtype=bool)
        one[p] = True
        alone = be.triangulate_ransac(x, select=one, want_hyp=True, **opts)
        for name in FIELDS + ("hyp_inliers",):
            a, b = getattr(alone, name), getattr(first, name)
            if name == "inlier_mask":
                assert a[pi == p].tobytes() == b[pi == p].tobytes() and not a[pi != p].any(), (p, name)
            else:
                assert a[p].tobytes() == b[p].tobytes(), (p, name)
    # drawn pairs too: alone and in the batch the key is the point's index in the problem
    drawn = be.triangulate_ransac(x, want_hyp=True, max_pairs=16, seed=5)
    for p in (3 * EDGE_LENGTHS.index(12) + 1, 3 * EDGE_LENGTHS.index(65) + 1):
        one = np.zeros(P, dtype=bool)
        one[p] = True
        alone = be.triangulate_ransac(x, select=one, want_hyp=True, max_pairs=16, seed=5)
        assert alone.hyp_inliers[p].tobytes() == drawn.hyp_inliers[p].tobytes() and alone.points[p].tobytes() == drawn.points[p].tobytes()
    # the points in another order (observations of a point keep theirs): every point the same bits
    perm = np.random.default_rng(8).permutation(P)               # new index -> old point
    new_of = np.argsort(perm)
    o = np.argsort(new_of[pi], kind="stable")
    xs = np.concatenate([x[:6 * C], x[6 * C:].reshape(P, 3)[perm].ravel()])
    set_problem(be, (C, P, ci[o], new_of[pi][o], uv[o], K))
    sh = be.triangulate_ransac(xs, want_hyp=True, **opts)
    for name in FIELDS + ("hyp_inliers",):
        a, b = getattr(sh, name), getattr(first, name)
        assert a.tobytes() == (b[o] if name == "inlier_mask" else b[perm]).tobytes(), name


def test_camera_rows_read_through_l2(be, edges):
    """The form of problems whose camera table does not fit the LDS (forms.lds_tab = 0), forced on a fresh handle, in both
    storage precisions, against the restatement; the integers also against the staged form's."""
    import sfmba
    x, args, where = edges
    opts = dict(max_pairs=20, seed=4)
    b = sfmba.Backend(0)
    try:
        b.debug_option("tab_lds", 0)
        assert opts in trr.EDGE_OPTIONS
        for bits, case in ((64, "edges"), (32, "edges_f32")):
            stored = args if bits == 64 else args[:4] + (args[4].astype(np.float32).astype(np.float64),) + args[5:]
            ref = reference(x, stored, **opts)
            set_problem(be, args, bits)
            set_problem(b, args, bits)
            assert be.form("lds_tab") == 1 and b.form("lds_tab") == 0
            staged, direct = be.triangulate_ransac(x, want_hyp=True, **opts), b.triangulate_ransac(x, want_hyp=True, **opts)
            assert check_against(direct, ref, case, f"rows through L2, {bits} bits") >= len(ref["status"]) - 3
            if not ref["hyp_close"].any():
                for name in ("status", "views", "inliers", "best", "inlier_mask", "hyp_inliers"):
                    assert getattr(staged, name).tobytes() == getattr(direct, name).tobytes(), (bits, name)
    finally:
        be.set_precision(64)
        b.close()


@pytest.mark.parametrize("C", [670, 700])
def test_camera_tables_round_64_kib(be, C):
    """The staged R|T table is 96 bytes a camera: 670 cameras stay below 64 KiB of dynamic LDS and pass it together with the
    kernel's static LDS, 700 pass it alone -- the two sizes at which the launch asks for the large-LDS opt-in for a reason
    of its own.  (Bounds borrowed from "arc": the same generator with more cameras on the arc.)"""
    x, args, _ = trr.arc_scene(n_tracks=42, seed=31, lengths=[3, 4, 5] * 14, n_cameras=C, contaminate=False)
    table = 96 * C
    assert (table <= 65536 < table + 3152) if C == 670 else table > 65536
    set_problem(be, args)
    assert be.form("lds_tab") == 1
    res = be.triangulate_ransac(x, want_hyp=True)
    assert check_against(res, reference(x, args), "arc", f"{C} cameras") >= 40


# ---- test 8: isolation ------------------------------------------------------------------------------------------------------------

def test_robust_triangulation_does_not_disturb_a_solve():
    import sfmba
    pb = sfmba.make_problem(8, 120, 900, seed=21)
    use = np.arange(pb.n_obs) % 3 != 0

    def solve(b, before=False, between=False):
        b.set_precision(64)
        b.set_problem(*pb.args)
        if before:
            b.triangulate_ransac(pb.x_true, obs_use=use, max_pairs=8, want_hyp=True)
        opt = b.default_options()
        opt.ftol = 1e-10
        xs, res, _, _ = b.solve(pb.x0, opt, want_fun=False, want_grad=False)     # fun, grad stay on the device
        if between:
            kept = b.fetch_fun_grad()
            b.triangulate_ransac(pb.x0, select=np.arange(120) % 2 == 0)          # at ANOTHER x than the solve's result
            after = b.fetch_fun_grad()
            assert kept[0].tobytes() == after[0].tobytes() and kept[1].tobytes() == after[1].tobytes()
        fun, grad = b.fetch_fun_grad()
        return xs, res.cost, int(res.nfev), fun, grad, b.pcg_history()

    results = []
    for kw in (dict(), dict(between=True), dict(before=True)):
        b = sfmba.Backend(0)
        try:
            results.append(solve(b, **kw))
        finally:
            b.close()
    want = results[0]
    for got in results[1:]:
        assert got[0].tobytes() == want[0].tobytes() and got[1] == want[1] and got[2] == want[2]
        assert got[3].tobytes() == want[3].tobytes() and got[4].tobytes() == want[4].tobytes() and got[5] == want[5]


# ---- test 10: reconstruct(robust_triangulation=True) ----------------------------------------------------------------------------

class Scene:
    """The construction of tests/test_gpu_reconstruct.py: a ring of ten cameras round 300 points, one observation per
    (point, camera), shuffled feature rows, one match edge per image pair that shares points.  `graft`: that many tracks
    of five views or more that cameras 0 and 1 do not both see get one wrong feature -- the pixel of one observation
    moved by 50-200 px before the feature lists are built."""

    def __init__(self, graft):
        import sfmba
        from sfmba import api
        pb = sfmba.make_ring_problem(10, 300, 3000, seed=3)
        self.K = pb.K
        C = pb.n_cameras
        ci, pi, uv = np.asarray(pb.camera_indices), np.asarray(pb.point_indices), np.asarray(pb.points_2d, dtype=np.float64)
        _, firsts = np.unique(pi * C + ci, return_index=True)
        firsts.sort()
        self.ci, self.pi, self.uv = ci[firsts], pi[firsts], uv[firsts].copy()
        rng = np.random.default_rng(8)
        views = np.bincount(self.pi, minlength=300)
        both = np.intersect1d(self.pi[self.ci == 0], self.pi[self.ci == 1])
        cand = np.setdiff1d(np.flatnonzero(views >= 5), both)
        self.grafted_tracks = rng.choice(cand, size=graft, replace=False)
        self.grafted = np.zeros(len(self.ci), dtype=bool)
        for p in self.grafted_tracks:
            k = rng.choice(np.flatnonzero(self.pi == p))
            ang, far = rng.uniform(0.0, 2.0 * np.pi), rng.uniform(50.0, 200.0)
            self.uv[k] += [far * np.cos(ang), far * np.sin(ang)]
            self.grafted[k] = True
        self.feats = [rng.permutation(np.flatnonzero(self.ci == c)) for c in range(C)]
        row_of = np.empty(len(self.ci), dtype=np.int64)
        for f in self.feats:
            row_of[f] = np.arange(len(f))
        self.obs_of_feat = np.concatenate(self.feats)                # global feature id -> observation
        self.pts = [self.uv[f] for f in self.feats]
        cams = pb.x_true[:6 * C].reshape(C, 6)
        Rm = [api._matrix_from_rotvec(cams[c, :3]) for c in range(C)]
        Kinv = np.linalg.inv(self.K)
        self.matches = []
        for u in range(C):
            for v in range(u):
                ou, ov = np.flatnonzero(self.ci == u), np.flatnonzero(self.ci == v)
                common, iu, iv = np.intersect1d(self.pi[ou], self.pi[ov], return_indices=True)
                if len(common) == 0:
                    continue
                pairs = np.stack([row_of[ou[iu]], row_of[ov[iv]]], axis=1)
                Rrel, trel = Rm[v] @ Rm[u].T, Rm[v] @ (cams[u, 3:] - cams[v, 3:])
                tx = np.array([[0.0, -trel[2], trel[1]], [trel[2], 0.0, -trel[0]], [-trel[1], trel[0], 0.0]])
                E = tx @ Rrel
                self.matches.append((u, v, pairs, Kinv.T @ E @ Kinv, E))

    def final_observations(self, rec):
        kept = np.zeros(len(self.ci), dtype=bool)
        kept[self.obs_of_feat[rec.obs_feat]] = True
        return kept

    def point_known(self, rec):
        """(300, bool): the scene's point has a known track in the reconstruction."""
        t = rec.tracks
        point_of_track = self.pi[self.obs_of_feat[t.track_feat[t.track_ptr[:-1]]]]
        out = np.zeros(300, dtype=bool)
        out[point_of_track[rec.known]] = True
        return out


def test_reconstruct_with_robust_triangulation(be):
    import sfmba
    scene = Scene(graft=12)
    assert scene.grafted.sum() == 12
    kw = dict(init=(1, 0), batch=0, backend=be, filter=True, filter_options=dict(max_error_px=4.0))
    off = sfmba.reconstruct(scene.matches, scene.pts, scene.K, **kw)
    on = sfmba.reconstruct(scene.matches, scene.pts, scene.K, robust_triangulation=True, **kw)
    assert off.registered.all() and on.registered.all()
    k_off, k_on = scene.point_known(off), scene.point_known(on)
    f_off, f_on = scene.final_observations(off), scene.final_observations(on)
    g = scene.grafted_tracks
    print(f"known points: flag off {int(k_off.sum())}, on {int(k_on.sum())}; grafted tracks known: off {int(k_off[g].sum())}, "
          f"on {int(k_on[g].sum())}; grafted observations in the final set: off {int(f_off[scene.grafted].sum())}, "
          f"on {int(f_on[scene.grafted].sum())}")
    assert k_on.sum() > k_off.sum() and k_on[g].sum() >= 10 and k_off[g].sum() <= 2
    assert not f_on[scene.grafted].any()                         # every grafted observation was dropped
    # no clean observation of a kept point went with the triangulation step: a grafted track that is known keeps all its
    # other observations, and what both runs know keeps in the robust run everything the plain run keeps
    clean_of_kept = ~scene.grafted & k_on[scene.pi] & np.isin(scene.pi, g)
    assert f_on[clean_of_kept].all()
    common = ~scene.grafted & (k_on & k_off)[scene.pi]
    assert not np.any(f_off[common] & ~f_on[common])


# ---- test 11 and the errors -------------------------------------------------------------------------------------------------------

def test_errors_and_timing(be, cases):
    x, args, planted, options, ref = cases["arc_h10"]
    set_problem(be, args)
    for kw in (dict(threshold=np.nan), dict(min_depth=np.nan), dict(min_pair_angle_deg=np.nan), dict(xtol=np.nan),
               dict(min_angle_deg=np.nan), dict(max_error_px=np.nan), dict(max_pairs=0), dict(seed=-1)):
        with pytest.raises(ValueError):
            be.triangulate_ransac(x, **kw)
    with pytest.raises(TypeError):
        be.triangulate_ransac(x, max_iters=3)
    with pytest.raises(ValueError):
        be.triangulate_ransac(x, select=np.ones(4, dtype=bool))
    with pytest.raises(ValueError):
        be.triangulate_ransac(x, want_hyp=True, max_pairs=2 ** 31 // args[1] + 1)      # P * H >= 2^31
    timed = be.triangulate_ransac(x, profile=1, **options)
    assert np.isfinite(timed.kernel_us) and timed.kernel_us > 0.0
    assert be.triangulate_ransac(x, **options).kernel_us == 0.0
    us = be.time_kernel(x, 19, 3)
    assert np.isfinite(us) and us > 0.0
    print(f"entry 19: {us:.1f} us; entry 15: {be.time_kernel(x, 15, 3):.1f} us ({args[1]} points, {len(args[2])} observations)")
    import sfmba
    res = sfmba.triangulate_tracks_ransac(x, args, backend=be, **options)
    assert res.status.tobytes() == be.triangulate_ransac(x, **options).status.tobytes()
