"""GPU tests of sfmba_essential_ransac (k_ess_ransac, k_ess_finish), of find_essential_mat and of
select_initial_pair(two_view="essential"), against the numpy restatement (tests/essential_ref.py; there is no reference
code for E).

Bounds.  Counts, masks, the best hypothesis, status and the number of real roots are compared EXACTLY.  Two kinds of
hypothesis are left out: (a) one with a pair within 1e-9 x threshold of the threshold for a candidate that can decide,
(b) one whose two numpy routes (eigh of A^T A, SVD of A) disagree in root count or best count; at most 5 % of the
hypotheses of a case may be left out (the restatement alone leaves out 0 of them: tests/test_host_essential.py).  An edge
whose best hypothesis could change with one that was left out is not compared in its per-edge fields.
E itself: up to sign, against the restatement's candidate and against the true E, per edge within 1000 x the distance of
the two numpy routes on that very sample, floored at 1e-10: that distance is the reference's own measure of the sample's
conditioning, and the device (Jacobi on A^T A, bracketed roots) is a third route.  Backward errors (epipolar residual of
the five pairs, the trace constraint): 100 x the largest value the restatement reaches on the same inputs
(tests/golden/essential_bounds.json, written by tools/gen_essential_golden.py).  The pose of the end-to-end scene: twice
the restatement's error on the same input (the same file)."""
import functools
import json
import os

import numpy as np
import pytest

import essential_ref as er
import two_view_ref as tv
from conftest import ROOT
from kernel_source import kernel_constant

pytestmark = pytest.mark.gpu

K = er.K_TEST
EST_FIELDS = ("E", "inlier_mask", "inliers", "best", "best_root", "success", "status", "hyp_inliers", "hyp_roots")
F_FIELDS = ("F", "F_refit", "inlier_mask", "inliers", "best", "success", "status", "hyp_inliers")
H_FIELDS = ("H", "H_refit", "inlier_mask", "refit_mask", "inliers", "refit_inliers", "best", "success", "status", "hyp_inliers")
BOUNDS = json.load(open(os.path.join(ROOT, "tests", "golden", "essential_bounds.json")))


@pytest.fixture(scope="module")
def be():
    import sfmba
    b = sfmba.Backend(0)
    yield b
    b.close()


@functools.lru_cache(maxsize=None)
def count_cases():
    """The inputs of test 1 with the restatement's expectation, computed once."""
    return [(name, p1, p2, ptr, H, seed, er.count_expectation(p1, p2, ptr, H, seed)) for name, p1, p2, ptr, H, seed in er.count_cases()]


def same_bits(a, b, fields):
    for name in fields:
        x, y = getattr(a, name), getattr(b, name)
        assert (x is None and y is None) or x.tobytes() == y.tobytes(), name


def compare_counts(est, p1, p2, ptr, samples, expect, H, what):
    """A device result against the restatement -> the number of hypotheses left out."""
    left_out = 0
    for e, ref in enumerate(expect):
        sl = slice(int(ptr[e]), int(ptr[e + 1]))
        keep = ~ref["skip"]
        left_out += int(ref["skip"].sum())
        assert np.array_equal(est.hyp_inliers[e][keep], ref["hyp"][keep]), (what, e, np.flatnonzero(est.hyp_inliers[e] != ref["hyp"]))
        assert np.array_equal(est.hyp_roots[e][keep], ref["roots"][keep]), (what, e, np.flatnonzero(est.hyp_roots[e] != ref["roots"]))
        if ref["skip"].any() and ref["hyp"][ref["skip"]].max() >= ref["hyp"][keep].max(initial=-1) - 1:
            continue                                             # a hypothesis left out could be the best
        assert est.status[e] == ref["status"] and est.best[e] == ref["best"] and est.inliers[e] == ref["inliers"], (what, e)
        assert np.array_equal(est.inlier_mask[sl], ref["mask"]) and bool(est.success[e]) == ref["success"], (what, e)
        if ref["status"] == er.OK:
            # (candidates of equal count: which has the lowest z depends on the basis of the null space, so any of them)
            idx = samples[e][ref["best"]]
            Es, _ = er.candidates(p1[sl][idx], p2[sl][idx], K)
            ties = [c for c in Es if er.score_hypothesis([c], K, p1[sl], p2[sl], er.THRESHOLD)[0] == ref["inliers"]]
            assert er.nearest(ties, est.E[e])[1] <= 1e-6 and abs(np.linalg.norm(est.E[e]) - 1.0) <= 1e-15, (what, e)
            assert 0 <= est.best_root[e] < est.hyp_roots[e][est.best[e]]
        else:
            assert not est.E[e].any(), (what, e)
    return left_out


# ---- 1: counts, with caller-given and with device-drawn samples ------------------------------------------------------------
@pytest.mark.parametrize("case", (0, 1))
def test_counts_masks_and_roots_against_the_restatement(be, case):
    name, p1, p2, ptr, H, seed, expect = count_cases()[case]
    n_edges = len(ptr) - 1
    drawn = be.essential_ransac(p1, p2, K, edge_ptr=ptr, threshold=er.THRESHOLD, max_iters=H, seed=seed, want_hyp=True)
    sizes = [int(ptr[e + 1] - ptr[e]) for e in range(n_edges)]
    samples = np.stack([er.draw_samples5(seed, e, H, n) if n >= 5 else np.zeros((H, 5), dtype=np.int32) for e, n in enumerate(sizes)])
    given = be.essential_ransac(p1, p2, K, edge_ptr=ptr, samples=samples, threshold=er.THRESHOLD, want_hyp=True)
    same_bits(drawn, given, EST_FIELDS)
    left_out = compare_counts(drawn, p1, p2, ptr, samples, expect, H, name)
    total = H * sum(1 for e in range(n_edges) if ptr[e + 1] - ptr[e] >= 5)
    print(f"{name}: left out {left_out} of {total} hypotheses; roots {np.bincount(drawn.hyp_roots[drawn.hyp_roots >= 0], minlength=11).tolist()}")
    assert left_out <= 0.05 * total
    roots = drawn.hyp_roots[drawn.hyp_roots >= 0]
    assert roots.max() <= 10 and np.all(roots % 2 == 0)
    if name == "sizes":
        assert drawn.status[0] == drawn.FEW_PAIRS and drawn.best[0] == -1 and drawn.best_root[0] == -1 and drawn.inliers[0] == 0
        assert np.all(drawn.hyp_inliers[0] == -1) and np.all(drawn.hyp_roots[0] == -1) and not drawn.E[0].any()
        assert not drawn.inlier_mask[:4].any() and drawn.n_ok == n_edges - 1


# ---- 2, 3: E itself and its backward errors ---------------------------------------------------------------------------------
def test_estimates_within_the_conditioning_of_their_sample_and_backward_errors(be):
    p1, p2, ptr, Et = er.exact_cases()
    n_edges = len(Et)
    samples = np.tile(np.arange(5, dtype=np.int32), (n_edges, 1, 1))
    est = be.essential_ransac(p1, p2, K, edge_ptr=ptr, samples=samples, threshold=er.EXACT_THRESHOLD, want_hyp=True)
    assert est.n_ok == n_edges and np.all(est.inliers == 8) and np.all(est.best == 0) and np.all(est.hyp_inliers == 8)
    worst, epi, trace = 0.0, 0.0, 0.0
    for e in range(n_edges):
        a, b = p1[ptr[e]:ptr[e] + 5], p2[ptr[e]:ptr[e] + 5]
        routes, d_true, E_ref = er.route_distance(a, b, K, Et[e])
        bound = max(1000.0 * routes, 1e-10)
        d = max(er.sign_distance(est.E[e], E_ref), er.sign_distance(est.E[e], Et[e]))
        worst = max(worst, d / bound)
        assert d <= bound, (e, d, bound, routes, d_true)
        x, y = er.backward_errors(est.E[e], K, a, b)
        epi, trace = max(epi, x), max(trace, y)
    print(f"worst |E - reference| / bound: {worst:.3g}; epipolar {epi:.3g} (restatement {BOUNDS['backward']['epipolar']:.3g}), "
          f"trace {trace:.3g} (restatement {BOUNDS['backward']['trace']:.3g})")
    assert epi <= 100.0 * BOUNDS["backward"]["epipolar"] and trace <= 100.0 * BOUNDS["backward"]["trace"]


# ---- 4: edges ---------------------------------------------------------------------------------------------------------------
def test_statuses_repeated_samples_and_degenerate_input(be):
    rng = np.random.default_rng(2710)
    a, b = er.scene(rng, 40, K, "general", noise=0.3)[:2]
    # FEW_PAIRS at n = 4, through a mask too
    few = be.essential_ransac(a[:4], b[:4], K, max_iters=3, want_hyp=True)
    assert few.status[0] == few.FEW_PAIRS and few.n_ok == 0 and np.all(few.hyp_inliers == -1) and np.all(few.hyp_roots == -1)
    use = np.zeros(40, dtype=bool)
    use[[1, 5, 9, 30]] = True
    few = be.essential_ransac(a, b, K, pair_use=use, max_iters=3, want_hyp=True)
    assert few.status[0] == few.FEW_PAIRS and not few.inlier_mask.any() and few.best[0] == -1 and not few.E.any()
    # a repeated position is an invalid sample: -1; only such samples: DEGENERATE with best -1
    smp = np.array([[[0, 1, 2, 3, 4], [0, 1, 2, 3, 0], [5, 6, 7, 8, 9]]], dtype=np.int32)
    rep = be.essential_ransac(a, b, K, samples=smp, want_hyp=True)
    assert rep.hyp_inliers[0, 1] == -1 and rep.hyp_roots[0, 1] == -1 and rep.hyp_inliers[0, 0] >= 5 and rep.hyp_inliers[0, 2] >= 5
    rep = be.essential_ransac(a, b, K, samples=smp[:, 1:2], want_hyp=True)
    assert rep.status[0] == rep.DEGENERATE and rep.best[0] == -1 and rep.best_root[0] == -1 and rep.inliers[0] == 0
    assert not rep.inlier_mask.any() and not rep.E.any()
    # a position out of range: the call fails
    bad = smp.copy()
    bad[0, 0, 0] = 40
    with pytest.raises(ValueError, match="outside"):
        be.essential_ransac(a, b, K, samples=bad)
    # five collinear points in both images: no finite candidate or no root, count 0, DEGENERATE
    s = np.arange(5.0)
    line1 = np.stack([100.0 + 50.0 * s, 200.0 + 30.0 * s], axis=1)
    line2 = np.stack([150.0 + 40.0 * s, 180.0 + 35.0 * s], axis=1)
    col = be.essential_ransac(line1, line2, K, samples=np.arange(5, dtype=np.int32)[None, None], want_hyp=True)
    assert col.hyp_inliers[0, 0] == 0 and col.status[0] == col.DEGENERATE and not col.E.any() and col.inliers[0] == 0
    # H = 1 and an H that is no multiple of the slice: the slices of a one-edge batch against those of a wide batch
    one = be.essential_ransac(a, b, K, max_iters=1, seed=3, want_hyp=True)
    many = be.essential_ransac(a, b, K, max_iters=37, seed=3, want_hyp=True)
    assert one.hyp_inliers[0, 0] == many.hyp_inliers[0, 0] and one.hyp_roots[0, 0] == many.hyp_roots[0, 0]
    assert many.best[0] == int(np.argmax(many.hyp_inliers[0])) and many.inliers[0] == many.hyp_inliers[0].max()
    wide = [(a, b)] * 600                                        # 600 edges: one slice each
    ptr = np.arange(601, dtype=np.int64) * 40
    smp37 = er.draw_samples5(3, 0, 37, 40)
    w = be.essential_ransac(np.concatenate([x for x, _ in wide]), np.concatenate([y for _, y in wide]), K, edge_ptr=ptr,
                            samples=np.tile(smp37, (600, 1, 1)), want_hyp=True)
    for e in (0, 299, 599):
        assert w.hyp_inliers[e].tobytes() == many.hyp_inliers[0].tobytes() and w.hyp_roots[e].tobytes() == many.hyp_roots[0].tobytes()
        assert w.E[e].tobytes() == many.E[0].tobytes() and w.best[e] == many.best[0] and w.best_root[e] == many.best_root[0]
        assert w.inlier_mask[40 * e:40 * e + 40].tobytes() == many.inlier_mask.tobytes()


def test_hypothesis_counts_and_the_choice_between_slots(be):
    """Equal counts planted in two waves of one slice, in a later slice and in the last slot: the lowest h wins, and what
    it returns is what that sample returns alone.  One edge of 40 noise-free pairs, ten of them outliers; the planted
    sample is five clean pairs (the restatement: 4 real roots, 30 inliers), every other hypothesis a sample with an
    outlier (7 inliers)."""
    minslice = kernel_constant("kTwoViewMinSlice")
    H = 8 * minslice + 1                                         # nine slices of a one-edge batch on any grid
    rng = np.random.default_rng(2713)
    a, b, _, _, _, bad = er.scene(rng, 40, K, "general", noise=0.0, outliers=0.25)
    clean, dirty = np.flatnonzero(~bad), np.flatnonzero(bad)
    planted, filler = clean[:5].astype(np.int32), np.concatenate([clean[5:9], dirty[:1]]).astype(np.int32)
    ref = er.ransac_edge(a, b, K, np.stack([planted, filler]), er.THRESHOLD, margin=er.MARGIN)
    assert ref["roots"][0] > 0 and ref["hyp"][0] > ref["hyp"][1] >= 0 and not ref["near"].any()    # (else nothing below is a test)
    alone = be.essential_ransac(a, b, K, samples=planted[None, None], threshold=er.THRESHOLD, want_hyp=True)
    assert alone.status[0] == alone.OK and alone.hyp_inliers[0, 0] == ref["hyp"][0] and alone.best_root[0] >= 0

    def run(at):
        smp = np.tile(filler, (H, 1))
        smp[at] = planted
        est = be.essential_ransac(a, b, K, samples=smp[None], threshold=er.THRESHOLD, want_hyp=True)
        assert np.all(est.hyp_inliers[0][at] == ref["hyp"][0]) and np.all(np.delete(est.hyp_inliers[0], at) == ref["hyp"][1])
        assert np.all(est.hyp_roots[0][at] == alone.hyp_roots[0, 0])
        for name in ("E", "best_root", "inlier_mask", "inliers", "status", "success"):
            assert getattr(est, name).tobytes() == getattr(alone, name).tobytes(), (name, at)
        return est

    # h = 13 is met by an earlier wave of its slice than h = 10
    assert run([13, 10, 5 * minslice + 2, H - 1]).best[0] == 10
    assert run([H - 1]).best[0] == H - 1


def test_mask_batch_and_repeat_give_the_same_bits(be):
    rng = np.random.default_rng(2711)
    edges = [er.scene(rng, n, K, "general", noise=0.3, outliers=0.25)[:2] for n in (80, 150, 64, 200)]
    p1, p2, ptr = er.batch(edges)
    H = 40
    smp = np.stack([er.draw_samples5(6, e, H, 50) for e in range(4)])          # positions below 50: valid with and without the mask
    use = np.ones(len(p1), dtype=bool)
    use[rng.choice(len(p1), 60, replace=False)] = False
    for e in range(4):
        use[ptr[e]:ptr[e] + 50] = True
    masked = be.essential_ransac(p1, p2, K, edge_ptr=ptr, pair_use=use, samples=smp, want_hyp=True)
    kept = [(a[use[ptr[e]:ptr[e + 1]]], b[use[ptr[e]:ptr[e + 1]]]) for e, (a, b) in enumerate(edges)]
    q1, q2, qptr = er.batch(kept)
    removed = be.essential_ransac(q1, q2, K, edge_ptr=qptr, samples=smp, want_hyp=True)
    same_bits(masked, removed, [f for f in EST_FIELDS if f != "inlier_mask"])
    assert masked.inlier_mask[use].tobytes() == removed.inlier_mask.tobytes() and not masked.inlier_mask[~use].any()
    # two runs, and edge e of the batch as a one-edge batch
    one = be.essential_ransac(p1, p2, K, edge_ptr=ptr, samples=smp, profile=1, want_hyp=True)
    two = be.essential_ransac(p1, p2, K, edge_ptr=ptr, samples=smp, want_hyp=True)
    same_bits(one, two, EST_FIELDS)
    assert one.kernel_us > 0.0 and two.kernel_us == 0.0
    for e, (a, b) in enumerate(edges):
        part = be.essential_ransac(a, b, K, samples=smp[e:e + 1], want_hyp=True)
        for name in ("E", "inliers", "best", "best_root", "success", "status", "hyp_inliers", "hyp_roots"):
            assert getattr(part, name).tobytes() == getattr(one, name)[e:e + 1].tobytes(), (name, e)
        assert part.inlier_mask.tobytes() == one.inlier_mask[ptr[e]:ptr[e + 1]].tobytes()


# ---- 5: isolation -----------------------------------------------------------------------------------------------------------
def test_fundamental_and_homography_calls_beside_an_essential_call(be):
    rng = np.random.default_rng(2712)
    edges = [er.scene(rng, n, K, "general", noise=0.3, outliers=0.25)[:2] for n in (80, 150, 64)]
    p1, p2, ptr = er.batch(edges)
    kw = dict(edge_ptr=ptr, threshold=1.0, max_iters=40, seed=6, refit=1, want_hyp=True)
    f0, h0 = be.fundamental_ransac(p1, p2, **kw), be.homography_ransac(p1, p2, **kw)
    e0 = be.essential_ransac(p1, p2, K, edge_ptr=ptr, threshold=1.0, max_iters=40, seed=6, want_hyp=True)
    f1, h1 = be.fundamental_ransac(p1, p2, **kw), be.homography_ransac(p1, p2, **kw)
    e1 = be.essential_ransac(p1, p2, K, edge_ptr=ptr, threshold=1.0, max_iters=40, seed=6, want_hyp=True)
    same_bits(f0, f1, F_FIELDS)
    same_bits(h0, h1, H_FIELDS)
    same_bits(e0, e1, EST_FIELDS)
    assert e0.n_ok == 3


def test_essential_calls_need_no_problem_and_do_not_disturb_a_solve():
    import sfmba
    a, b = er.scene(np.random.default_rng(2713), 120, K, "general", noise=0.3, outliers=0.25)[:2]
    pb = sfmba.make_problem(6, 60, 400, seed=21)

    def solve(bk, beside):
        got = []
        if beside:
            got.append(bk.essential_ransac(a, b, K, max_iters=32, seed=1, want_hyp=True))      # no problem has been set yet
        bk.set_precision(64)
        bk.set_problem(*pb.args)
        opt = bk.default_options()
        opt.ftol = 1e-10
        xs, res, _, _ = bk.solve(pb.x0, opt, want_fun=False, want_grad=False)
        if beside:
            got.append(bk.essential_ransac(a, b, K, max_iters=32, seed=1, want_hyp=True))
        fun, grad = bk.fetch_fun_grad()
        return (xs, res.cost, int(res.nfev), fun, grad, bk.pcg_history()), got

    results = []
    for beside in (False, True):
        bk = sfmba.Backend(0)
        try:
            results.append(solve(bk, beside))
        finally:
            bk.close()
    want, got = results[0][0], results[1][0]
    assert got[0].tobytes() == want[0].tobytes() and got[1] == want[1] and got[2] == want[2]
    assert got[3].tobytes() == want[3].tobytes() and got[4].tobytes() == want[4].tobytes() and got[5] == want[5]
    same_bits(results[1][1][0], results[1][1][1], EST_FIELDS)
    assert results[1][1][0].status[0] == 0


# ---- 6: end to end ----------------------------------------------------------------------------------------------------------
def test_find_essential_mat_and_the_initial_pair(be):
    import sfmba
    g = BOUNDS["end_to_end"]
    p1, p2, R, t = er.noisy_scene()
    E, mask = sfmba.find_essential_mat(p1.reshape(-1, 1, 2), p2.reshape(-1, 1, 2), K, threshold=er.THRESHOLD, maxIters=g["H"],
                                       seed=g["seed"], backend=be)
    assert E.shape == (3, 3) and mask.shape == (300, 1) and mask.dtype == np.uint8 and set(np.unique(mask)) <= {0, 1}
    m = mask.ravel().astype(bool)
    n_front, Rd, td, front = sfmba.recover_pose(E, p1[m], p2[m], K, backend=be)
    rot, tdir = er.pose_errors(Rd, td.ravel(), R, t)
    print(f"inliers {int(m.sum())} (restatement {g['inliers']}), rotation {rot:.3g} rad (restatement {g['rotation_rad']:.3g}), "
          f"translation direction {tdir:.3g} rad (restatement {g['translation_rad']:.3g})")
    assert rot <= 2.0 * g["rotation_rad"] and tdir <= 2.0 * g["translation_rad"] and n_front >= 0.9 * m.sum()
    none, _ = sfmba.find_essential_mat(p1[:4], p2[:4], K, backend=be)
    assert none is None
    # the first pair
    gp = BOUNDS["initial_pair"]
    edges = er.pair_edges()
    got = sfmba.select_initial_pair(edges, K, backend=be, two_view="essential", threshold=er.THRESHOLD, max_iters=gp["H"], seed=gp["seed"])
    assert got[0] == gp["index"] and abs(np.linalg.det(got[1]) - 1.0) <= 1e-9 and abs(np.linalg.norm(got[2]) - 1.0) <= 1e-9
    gated = sfmba.select_initial_pair(edges, K, backend=be, two_view="essential", max_homography_ratio=0.8, threshold=er.THRESHOLD,
                                      max_iters=gp["H"], seed=gp["seed"])
    assert gated[0] == gp["index"]
    # the default keyword makes exactly the former calls
    kw = dict(threshold=er.THRESHOLD, max_iters=gp["H"], seed=gp["seed"])
    dflt = sfmba.select_initial_pair(edges, K, backend=be, **kw)
    named = sfmba.select_initial_pair(edges, K, backend=be, two_view="fundamental", **kw)
    q1, q2, ptr = er.batch(edges)
    est = be.fundamental_ransac(q1, q2, edge_ptr=ptr, refit=1, **kw)
    pose = be.recover_pose(np.einsum("ji,ejk,kl->eil", K, est.F_refit, K), q1, q2, K, edge_ptr=ptr, pair_use=est.inlier_mask)
    assert dflt[0] is not None and dflt[0] == named[0]
    for x, y in zip(dflt[1:], named[1:]):
        assert x.tobytes() == y.tobytes()
    assert dflt[1].tobytes() == pose.R[dflt[0]].tobytes() and dflt[2].tobytes() == pose.t[dflt[0]].tobytes()
    assert tv.rotation_angle(dflt[1], got[1]) < 1.0              # (radians: the two routes see the same scene)
