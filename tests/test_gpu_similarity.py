"""GPU tests of sfmba_similarity_ransac (k_sim_ransac, k_sim_finish), of estimate_similarity, align_reconstruction and
merge_reconstructions: against the numpy restatement (tests/similarity_ref.py, written from the header), the sizes at
which the kernels take another path, every status, masks, determinism, isolation from the F call and from the solver.

Bounds.  Counts, masks and the best hypothesis are compared EXACTLY; a hypothesis is left out of the comparison when the
restatement finds one of its distances within 1e-6 x threshold of the threshold (at most 1 % of them may be), and a set
with such a hypothesis, or with such a distance of its refit, is skipped for the per-set fields.  (s, R, t) and the refit:
the unit quaternion of Horn's N moves by |dN| / (l1 - l2) with |dN| = 64 eps |N|_F; R by twice that, s and t as
similarity_ref.estimate_tolerance carries it on.  Two numpy routes (Horn by eigh, Umeyama by SVD) differ by at most 0.0877
of it (tests/test_host_similarity.py).

What was measured on the MI355X is in the docstrings of the tests: left-out shares (none) and worst ratios."""
import numpy as np
import pytest

import similarity_ref as sr
import two_view_ref as tv
from kernel_source import kernel_constant

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
EST_FIELDS = ("scale", "R", "t", "scale_refit", "R_refit", "t_refit", "inlier_mask", "refit_mask", "inliers", "refit_inliers", "best",
              "success", "status", "hyp_inliers")
SET_FIELDS = ("scale", "R", "t", "scale_refit", "R_refit", "t_refit", "inliers", "refit_inliers", "best", "success", "status", "hyp_inliers")
F_FIELDS = ("F", "F_refit", "inlier_mask", "inliers", "best", "success", "status", "hyp_inliers")
NONE = (np.zeros((0, 3)), np.zeros((0, 3)))
THR = 0.05
WORST = dict(ratio=0.0)                                          # the largest |estimate - restatement| / bound met by any test


@pytest.fixture(scope="module")
def be():
    import sfmba
    b = sfmba.Backend(0)
    yield b
    b.close()


def batch(sets):
    """[(src, dst), ...] -> src, dst, set_ptr"""
    ptr = np.concatenate([[0], np.cumsum([len(a) for a, _ in sets])]).astype(np.int64)
    return (np.concatenate([a for a, _ in sets]).reshape(-1, 3), np.concatenate([b for _, b in sets]).reshape(-1, 3), ptr)


def same_bits(a, b, fields):
    for name in fields:
        x, y = getattr(a, name), getattr(b, name)
        assert (x is None and y is None) or x.tobytes() == y.tobytes(), name


def sim_of(est, e, refit=False):
    return (est.scale_refit[e], est.R_refit[e], est.t_refit[e]) if refit else (est.scale[e], est.R[e], est.t[e])


def is_zero(sim):
    return sim[0] == 0.0 and not sim[1].any() and not sim[2].any()


def proper(R):
    return np.abs(R @ R.T - np.eye(3)).max() <= 16 * EPS and abs(np.linalg.det(R) - 1.0) <= 16 * EPS


def check_set(est, e, a, b, samples, thr, refit=True, confidence=0.99):
    """Set e of a device result against the restatement on the same samples -> the number of hypotheses left out (a
    refit with a distance near the threshold counts as one)."""
    ref = sr.ransac_set(a, b, samples, thr, confidence=confidence, refit=refit, margin=1e-6 * thr)
    sl = slice(int(est.set_ptr[e]), int(est.set_ptr[e + 1]))
    keep = ~ref["near"]
    assert np.array_equal(est.hyp_inliers[e][keep], ref["hyp"][keep]), e
    if ref["near"].any():
        return int(ref["near"].sum())
    assert est.status[e] == ref["status"] and est.best[e] == ref["best"] and est.inliers[e] == ref["inliers"], e
    assert np.array_equal(est.inlier_mask[sl], ref["mask"]) and bool(est.success[e]) == ref["success"], e
    if ref["status"] != sr.OK:
        assert is_zero(sim_of(est, e)) and is_zero(sim_of(est, e, True)), e
        assert np.array_equal(est.refit_mask[sl], ref["mask"]) and est.refit_inliers[e] == ref["inliers"], e
        return 0
    idx = np.asarray(samples)[ref["best"]]
    ratio = sr.tolerance_ratio(sim_of(est, e), ref["sim"], a[idx], b[idx])
    WORST["ratio"] = max(WORST["ratio"], ratio)
    assert ratio <= 1.0 and proper(est.R[e]) and est.scale[e] > 0.0, (e, ratio)
    if not refit:
        same_bits_of = [(est.scale_refit, est.scale), (est.R_refit, est.R), (est.t_refit, est.t)]
        assert all(x[e].tobytes() == y[e].tobytes() for x, y in same_bits_of)
        assert est.refit_mask[sl].tobytes() == est.inlier_mask[sl].tobytes() and est.refit_inliers[e] == est.inliers[e]
        return 0
    m = ref["mask"]
    ratio = sr.tolerance_ratio(sim_of(est, e, True), ref["sim_refit"], a[m], b[m])
    WORST["ratio"] = max(WORST["ratio"], ratio)
    assert ratio <= 1.0 and proper(est.R_refit[e]), (e, ratio)
    if ref["near_refit"]:
        return 1
    assert np.array_equal(est.refit_mask[sl], ref["refit_mask"]) and est.refit_inliers[e] == ref["refit_inliers"], e
    return 0


# ---- 1: drawn samples against the restatement ---------------------------------------------------------------------------
def test_drawn_samples_against_the_restatement_and_e_dependence(be):
    """3 sets of 300 pairs, noise 0.01, threshold 0.05, 25 % outliers displaced by up to +-8, 100 drawn hypotheses each.
    On the CPU (the restatement): 0 of 300 hypotheses are near the threshold; the best counts are 225, 225 and 225, the
    number of clean pairs of each set.  On the MI355X: left out 0 of 300."""
    rng = np.random.default_rng(41)
    H, seed = 100, 0xfedcba9876543210
    made = [sr.similar_sets(rng, 300, noise=0.01, outliers=0.25) for _ in range(3)]
    sets = [m[:2] for m in made]
    src, dst, ptr = batch(sets)
    est = be.similarity_ransac(src, dst, set_ptr=ptr, threshold=THR, max_iters=H, seed=seed, refit=1, want_hyp=True)
    left_out = 0
    for e, (a, b) in enumerate(sets):
        smp = sr.draw_samples3(seed, e, H, len(a))
        left_out += check_set(est, e, a, b, smp, THR)
        # the documented e-dependence: set e of the batch is a one-set batch given that set's samples
        one = be.similarity_ransac(a, b, samples=smp[None], threshold=THR, refit=1, want_hyp=True)
        sl = slice(int(ptr[e]), int(ptr[e + 1]))
        for name in SET_FIELDS:
            assert getattr(one, name)[0].tobytes() == getattr(est, name)[e].tobytes(), name
        assert one.inlier_mask.tobytes() == est.inlier_mask[sl].tobytes() and one.refit_mask.tobytes() == est.refit_mask[sl].tobytes()
    print(f"left out: {left_out} of {3 * H} hypotheses; best counts {est.inliers.tolist()}, refit {est.refit_inliers.tolist()}")
    assert left_out <= 0.01 * 3 * H
    assert est.n_ok == 3 and est.inliers.tolist() == [int((~m[3]).sum()) for m in made]
    for e, m in enumerate(made):                                 # the scene's similarity, to the noise
        assert abs(est.scale_refit[e] - m[2][0]) < 1e-3 and np.abs(est.R_refit[e] - m[2][1]).max() < 1e-3
    # ... and drawn as set 0 of its own batch it differs from set 1 of this one
    other = be.similarity_ransac(*sets[1], threshold=THR, max_iters=H, seed=seed, want_hyp=True)
    assert other.hyp_inliers[0].tobytes() != est.hyp_inliers[1].tobytes()


# ---- 2: (s, R, t) and the refit within the bound of the estimate's own conditioning ---------------------------------------
def test_estimates_within_the_bound_of_their_conditioning(be):
    """Measured on the MI355X: worst |estimate - restatement| / bound over 30 estimates 0.0198, none left out."""
    rng = np.random.default_rng(42)
    sets = []
    for n in (3, 4, 9, 64, 300):
        noise = 0.0 if n <= 4 else 0.01
        sets.append(sr.similar_sets(rng, n, noise=noise)[:2])
        sets.append(sr.similar_sets(rng, n, noise=noise, scale=250.0, spread=0.5)[:2])     # far from the origin, large scale
        sets.append(sr.similar_sets(rng, n, noise=noise, angle=3.14)[:2])
    src, dst, ptr = batch(sets)
    H, seed = 16, 5
    before = WORST["ratio"]
    WORST["ratio"] = 0.0
    est = be.similarity_ransac(src, dst, set_ptr=ptr, threshold=THR, max_iters=H, seed=seed, refit=1, want_hyp=True)
    left_out = sum(check_set(est, e, a, b, sr.draw_samples3(seed, e, H, len(a)), THR) for e, (a, b) in enumerate(sets))
    print(f"worst |estimate - restatement| / bound over {2 * len(sets)} estimates: {WORST['ratio']:.4f}; left out {left_out}")
    assert est.n_ok == len(sets) and left_out <= 0.01 * H * len(sets) and 0.0 < WORST["ratio"] <= 1.0
    WORST["ratio"] = max(WORST["ratio"], before)


# ---- 3: sizes at which a path changes ---------------------------------------------------------------------------------------
def test_pair_counts_at_the_edges_of_the_loops(be):
    """n = 2 (FEW_PAIRS), 3, 4 (exact data: every pair fits), around the wave's 64, and at the LDS staging limit and one
    above it (read from global memory), in one batch with an empty set in the middle."""
    L = kernel_constant("kSimLdsPairs")
    rng = np.random.default_rng(43)
    sizes = [2, 3, 4, 63, 0, 64, 65, L, L + 1]
    sets = [sr.similar_sets(rng, n, noise=0.0 if n <= 4 else 0.01, outliers=0.0 if n <= 4 else 0.25)[:2] if n else NONE for n in sizes]
    src, dst, ptr = batch(sets)
    H, seed = 24, 77
    est = be.similarity_ransac(src, dst, set_ptr=ptr, threshold=THR, max_iters=H, seed=seed, refit=1, want_hyp=True)
    left_out = 0
    for e, n in enumerate(sizes):
        sl = slice(int(ptr[e]), int(ptr[e + 1]))
        if n < 3:
            assert est.status[e] == est.FEW_PAIRS and np.all(est.hyp_inliers[e] == -1) and est.best[e] == -1
            assert is_zero(sim_of(est, e)) and is_zero(sim_of(est, e, True)) and est.inliers[e] == 0 and est.refit_inliers[e] == 0
            assert not est.inlier_mask[sl].any() and not est.refit_mask[sl].any() and not est.success[e]
            continue
        left_out += check_set(est, e, *sets[e], sr.draw_samples3(seed, e, H, n), THR)
    print(f"left out: {left_out} of {H * len(sizes)} hypotheses")
    assert left_out <= 0.01 * H * len(sizes)
    assert est.n_ok == int((est.status == est.OK).sum()) == 7
    assert est.inliers[1] == 3 and est.inliers[2] == 4 and np.all(est.hyp_inliers[1] == 3)      # exact data: every pair fits


# ---- 4: hypothesis counts and the choice between lanes, rounds, waves and slots ------------------------------------------
def test_hypothesis_counts_and_the_choice_between_slots(be):
    minslice = kernel_constant("kSimMinSlice")
    rng = np.random.default_rng(44)
    a, b, _, bad = sr.similar_sets(rng, 64, noise=0.0, outliers=0.25)
    big = 8 * minslice + 1                                       # nine slices of a one-set batch on any grid
    for H in sorted({1, 3, 63, 64, 65, minslice - 1, minslice + 1, big}):
        est = be.similarity_ransac(a, b, threshold=THR, max_iters=H, seed=3, want_hyp=True)
        assert check_set(est, 0, a, b, sr.draw_samples3(3, 0, H, 64), THR, refit=False) == 0
    H = big
    clean, dirty = np.flatnonzero(~bad), np.flatnonzero(bad)
    smp = np.empty((H, 3), dtype=np.int32)
    for h in range(H):                                           # every sample holds an outlier ...
        smp[h] = np.concatenate([rng.choice(clean, 2, replace=False), rng.choice(dirty, 1)])
    smp[H - 1] = clean[:3]                                       # ... but the last
    est = be.similarity_ransac(a, b, samples=smp[None], threshold=THR, want_hyp=True)
    assert check_set(est, 0, a, b, smp, THR, refit=False) == 0
    assert est.best[0] == H - 1 and est.inliers[0] == len(clean) and np.array_equal(est.inlier_mask, ~bad)
    # the same sample, so the same count, at several h of a one-set batch (nine slices of one round of one wave each): two
    # lanes of one slice, other slices, the last slot -- the lowest h wins
    one = smp.copy()
    hs = (H + 8) // 9
    for h in (13, 10, 5 * hs + 2, H - 6):
        one[h] = clean[:3]
    est = be.similarity_ransac(a, b, samples=one[None], threshold=THR, want_hyp=True)
    assert np.all(est.hyp_inliers[0][[10, 13, 5 * hs + 2, H - 6, H - 1]] == len(clean))
    assert est.best[0] == 10 and check_set(est, 0, a, b, one, THR, refit=False) == 0
    # a batch of so many sets that each has ONE slice (at least two workgroups a CU without slicing): all four waves and
    # three rounds.  Two lanes of one round of wave 1 (h = 70, 67), a later round of wave 0 (256 + 5), wave 2 (130), the last
    many = 1024
    for h in (70, 67, 256 + 5, 130):
        smp[h] = clean[:3]
    src, dst, ptr = batch([(a, b)] * many)
    est = be.similarity_ransac(src, dst, set_ptr=ptr, samples=np.broadcast_to(smp, (many, H, 3)), threshold=THR, want_hyp=True)
    assert np.all(est.hyp_inliers[:, [67, 70, 130, 256 + 5, H - 1]] == len(clean)) and np.all(est.best == 67)
    assert check_set(est, 0, a, b, smp, THR, refit=False) == 0 and check_set(est, many - 1, a, b, smp, THR, refit=False) == 0
    for name in SET_FIELDS:
        v = getattr(est, name)
        assert all(v[e].tobytes() == v[0].tobytes() for e in (1, many // 2, many - 1)), name


# ---- 5: caller samples ------------------------------------------------------------------------------------------------------
def test_repeated_degenerate_and_out_of_range_samples_and_refit_off(be):
    rng = np.random.default_rng(45)
    a, b = sr.similar_sets(rng, 30)[:2]
    smp = sr.draw_samples3(4, 0, 12, 30)
    smp[5, 2] = smp[5, 0]
    est = be.similarity_ransac(a, b, samples=smp[None], threshold=THR, want_hyp=True)
    assert est.hyp_inliers[0][5] == -1 and np.all(np.delete(est.hyp_inliers[0], 5) == 30) and est.best[0] == 0
    assert est.status[0] == est.OK
    # refit = 0 (the default): copies
    assert est.scale_refit.tobytes() == est.scale.tobytes() and est.R_refit.tobytes() == est.R.tobytes()
    assert est.t_refit.tobytes() == est.t.tobytes() and est.refit_mask.tobytes() == est.inlier_mask.tobytes()
    assert est.refit_inliers.tobytes() == est.inliers.tobytes()
    # every sample repeated: DEGENERATE with no best hypothesis
    rep = np.tile(np.array([[1, 2, 1]], dtype=np.int32), (12, 1))
    deg = be.similarity_ransac(a, b, samples=rep[None], threshold=THR, refit=1, want_hyp=True)
    assert deg.status[0] == deg.DEGENERATE and deg.best[0] == -1 and np.all(deg.hyp_inliers[0] == -1) and deg.n_ok == 0
    assert is_zero(sim_of(deg, 0)) and is_zero(sim_of(deg, 0, True)) and not deg.inlier_mask.any() and not deg.refit_mask.any()
    assert deg.inliers[0] == 0 and deg.refit_inliers[0] == 0 and not deg.success[0]
    # a collinear source triple and a thrice-repeated point: the samples are valid, they have no solution
    line = a.copy()
    line[:3] = a[0] + np.outer([0.0, 1.0, 2.5], a[1] - a[0])
    for s3, d3 in ((line, b), (np.tile(a[:1], (20, 1)), np.tile(b[:1], (20, 1)))):
        flat = be.similarity_ransac(s3, d3, samples=np.tile(np.array([[0, 1, 2]], dtype=np.int32), (1, 8, 1)), threshold=THR,
                                    refit=1, want_hyp=True)
        assert flat.status[0] == flat.DEGENERATE and np.all(flat.hyp_inliers[0] == 0) and flat.best[0] == 0
        assert is_zero(sim_of(flat, 0)) and is_zero(sim_of(flat, 0, True)) and flat.inliers[0] == 0 and not flat.inlier_mask.any()
    # a position out of range: the call returns -1, which the binding raises as ValueError as for every call
    for bad in (30, -1):
        smp2 = smp.copy()
        smp2[3, 2] = bad
        with pytest.raises(ValueError, match="position"):
            be.similarity_ransac(a, b, samples=smp2[None], threshold=THR)
    with pytest.raises(ValueError):
        be.similarity_ransac(a, b, max_iters=0)
    with pytest.raises(ValueError):
        be.similarity_ransac(a, b, threshold=np.nan)
    with pytest.raises(TypeError):
        be.similarity_ransac(a, b, iterations=3)
    with pytest.raises(ValueError):
        be.similarity_ransac(a, b, samples=smp[None], max_iters=11)
    with pytest.raises(ValueError):
        be.similarity_ransac(a, b, samples=np.zeros((1, 12, 4), dtype=np.int32))
    # the handle is still good
    assert be.similarity_ransac(a, b, samples=smp[None], threshold=THR).inliers[0] == 30


# ---- 6: a mask --------------------------------------------------------------------------------------------------------------
def test_pair_use_equals_the_batch_without_those_pairs(be):
    rng = np.random.default_rng(46)
    made = [sr.similar_sets(rng, n, noise=0.01, outliers=0.25) for n in (90, 70)]
    src, dst, ptr = batch([(m[0], m[1]) for m in made])
    use = rng.uniform(size=len(src)) > 0.3
    use[ptr[1] - 1] = False
    kept_ptr = np.array([0, use[:ptr[1]].sum(), use.sum()], dtype=np.int64)
    smp = np.stack([sr.draw_samples3(9, e, 24, int(kept_ptr[e + 1] - kept_ptr[e])) for e in range(2)])
    for kw in (dict(samples=smp), dict(max_iters=24, seed=9)):
        full = be.similarity_ransac(src, dst, set_ptr=ptr, pair_use=use, threshold=THR, refit=1, want_hyp=True, **kw)
        cut = be.similarity_ransac(src[use], dst[use], set_ptr=kept_ptr, threshold=THR, refit=1, want_hyp=True, **kw)
        same_bits(full, cut, SET_FIELDS)
        assert np.array_equal(full.inlier_mask[use], cut.inlier_mask) and not full.inlier_mask[~use].any()
        assert np.array_equal(full.refit_mask[use], cut.refit_mask) and not full.refit_mask[~use].any()
        assert cut.n_ok == 2 and cut.refit_inliers.min() >= 20


# ---- 7: determinism and isolation -------------------------------------------------------------------------------------------
def test_same_bits_twice_beside_the_fundamental_call_and_in_two_parts(be):
    rng = np.random.default_rng(47)
    sets = [sr.similar_sets(rng, n, noise=0.01, outliers=0.25)[:2] for n in (80, 150, 64, 200)]
    src, dst, ptr = batch(sets)
    Kc = np.array([[2905.88, 0.0, 1416.0], [0.0, 2905.88, 1064.0], [0.0, 0.0, 1.0]])
    p1, p2 = tv.make_pairs(rng, 120, Kc, noise=0.3, outliers=0.25)[:2]
    kw = dict(set_ptr=ptr, threshold=THR, max_iters=40, seed=6, refit=1, want_hyp=True)
    fkw = dict(threshold=1.0, max_iters=40, seed=6, refit=1, want_hyp=True)
    f0 = be.fundamental_ransac(p1, p2, **fkw)
    one = be.similarity_ransac(src, dst, profile=1, **kw)
    f1 = be.fundamental_ransac(p1, p2, **fkw)
    two = be.similarity_ransac(src, dst, **kw)
    same_bits(one, two, EST_FIELDS)
    same_bits(f0, f1, F_FIELDS)
    assert one.kernel_us > 0.0 and two.kernel_us == 0.0 and one.n_ok == 4
    # the batch in two parts, the samples passed along
    smp = np.stack([sr.draw_samples3(6, e, 40, len(sets[e][0])) for e in range(4)])
    for lo, hi in ((0, 1), (1, 4)):
        q1, q2, qptr = batch(sets[lo:hi])
        part = be.similarity_ransac(q1, q2, set_ptr=qptr, samples=smp[lo:hi], threshold=THR, refit=1, want_hyp=True)
        for name in SET_FIELDS:
            assert getattr(part, name).tobytes() == getattr(one, name)[lo:hi].tobytes(), name
        assert part.inlier_mask.tobytes() == one.inlier_mask[int(ptr[lo]):int(ptr[hi])].tobytes()
        assert part.refit_mask.tobytes() == one.refit_mask[int(ptr[lo]):int(ptr[hi])].tobytes()


def test_similarity_calls_need_no_problem_and_do_not_disturb_a_solve():
    import sfmba
    rng = np.random.default_rng(48)
    a, b = sr.similar_sets(rng, 120, noise=0.01, outliers=0.25)[:2]
    pb = sfmba.make_problem(6, 60, 400, seed=21)

    def solve(bk, beside):
        got = []
        if beside:
            got.append(bk.similarity_ransac(a, b, threshold=THR, max_iters=32, seed=1, refit=1))      # no problem has been set yet
        bk.set_precision(64)
        bk.set_problem(*pb.args)
        opt = bk.default_options()
        opt.ftol = 1e-10
        xs, res, _, _ = bk.solve(pb.x0, opt, want_fun=False, want_grad=False)          # fun, grad stay on the device
        if beside:
            got.append(bk.similarity_ransac(a, b, threshold=THR, max_iters=32, seed=1, refit=1))
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
    same_bits(results[1][1][0], results[1][1][1], EST_FIELDS[:-1])
    assert results[1][1][0].status[0] == 0


# ---- 8: a set without a common similarity -----------------------------------------------------------------------------------
def test_a_mirrored_set_is_ok_with_a_handful_of_inliers_and_estimate_similarity_says_none(be):
    """Every triangle is congruent to its mirror image, and a mirror image of a plane is a rotation of it: so every
    hypothesis fits its own three pairs and the raw call reports OK with that small count.  This is why the Python layer
    has min_inliers.  On the CPU (the restatement): the largest count of the 64 hypotheses is 4."""
    import sfmba
    rng = np.random.default_rng(49)
    a, b = sr.similar_sets(rng, 40)[:2]
    b = b * np.array([-1.0, 1.0, 1.0])
    est = be.similarity_ransac(a, b, threshold=THR, max_iters=64, seed=2, refit=1, want_hyp=True)
    assert check_set(est, 0, a, b, sr.draw_samples3(2, 0, 64, 40), THR) == 0
    assert est.status[0] == est.OK and 3 <= est.inliers[0] <= 5 and est.hyp_inliers[0].max() == est.inliers[0]
    s, R, t, mask = sfmba.estimate_similarity(a, b, threshold=THR, max_iters=64, seed=2, backend=be)
    assert s is None and R is None and t is None and mask.shape == (40,) and mask.sum() == est.refit_inliers[0] < 6
    # the same set unmirrored: the estimate, and its default threshold
    b = b * np.array([-1.0, 1.0, 1.0])
    s, R, t, mask = sfmba.estimate_similarity(a, b, max_iters=64, seed=2, backend=be)
    assert mask.all() and sr.distances_sq((s, R, t), a, b).max() < 1e-20 and proper(R)
    s0, R0, t0, mask0 = sfmba.estimate_similarity(a, b, max_iters=64, seed=2, refit=False, backend=be)
    assert mask0.all() and sr.distances_sq((s0, R0, t0), a, b).max() < 1e-18


# ---- 9: reconstructions -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene_and_rec(be):
    import sfmba
    from test_gpu_reconstruct import Scene
    scene = Scene()
    return scene, sfmba.reconstruct(scene.matches, scene.pts, scene.K, init=(1, 0), batch=0, backend=be)


def test_align_reconstruction_to_known_centres_with_two_wrong_ones(be, scene_and_rec):
    """The clean fit (the aligned() helper of tests/test_gpu_reconstruct.py over all ten true centres) leaves the centres
    within a distance that is measured here first; the robust fit, given two centres moved by 10 units, must leave the
    other eight within twice that.  Measured on the MI355X: clean 2.774e-03, robust 1.851e-03 scene units."""
    import sfmba
    from test_gpu_reconstruct import aligned
    scene, rec = scene_and_rec
    C = scene.pb.n_cameras
    true = scene.pb.x_true[:6 * C].reshape(C, 6)[:, 3:]
    assert rec.registered.all()
    x, args = rec.problem()
    clean = np.linalg.norm(aligned(x, args[0], true[rec.cam_of])[0] - true[rec.cam_of], axis=1).max()
    given = true.copy()
    moved = [2, 7]
    given[2] += [10.0, 0.0, 0.0]
    given[7] += [0.0, -6.0, 8.0]
    out, est = sfmba.align_reconstruction(rec, given, backend=be, seed=1)
    others = np.setdiff1d(np.arange(C), moved)
    robust = np.linalg.norm(out.cameras[others, 3:] - true[others], axis=1).max()
    print(f"centres after the clean fit within {clean:.3e}, after the robust fit within {robust:.3e} scene units")
    assert 0.0 < robust <= 2.0 * clean and clean < 0.05
    assert est.status[0] == est.OK and est.refit_mask.tolist() == [i not in moved for i in range(C)] and est.refit_inliers[0] == C - 2
    # the problem went along: same reprojections, and the points sit where the truth has them
    x2, args2 = out.problem()
    r0, r1 = sfmba.total_mean_reproj_error(x, args, backend=be), sfmba.total_mean_reproj_error(x2, args2, backend=be)
    assert abs(r1 - r0) <= 1e-9 * r0 and args2 is args
    assert np.array_equal(np.isnan(out.points), np.isnan(rec.points)) and np.array_equal(out.known, rec.known)
    truth = scene.truth_for(rec)[6 * C:].reshape(-1, 3)
    assert np.linalg.norm(out.points[rec.pt_of] - truth, axis=1).max() < 0.05
    # too few correspondences, too few inliers
    few = np.full((C, 3), np.nan)
    few[:5] = true[:5]
    with pytest.raises(ValueError, match="min_inliers"):
        sfmba.align_reconstruction(rec, few, backend=be)
    with pytest.raises(ValueError, match="min_inliers"):
        sfmba.align_reconstruction(rec, given, min_inliers=9, backend=be)
    with pytest.raises(ValueError):
        sfmba.align_reconstruction(rec, true[:5], backend=be)


def view(rec, images):
    """The part of a reconstruction that `images` hold: those cameras, and the known tracks that two or more of them see."""
    import sfmba
    t = rec.tracks
    track_id = np.repeat(np.arange(t.n_tracks), np.diff(t.track_ptr))
    seen = np.bincount(track_id[np.isin(t.track_image, images)], minlength=t.n_tracks) >= 2
    registered = np.zeros_like(rec.registered)
    registered[images] = True
    known = rec.known & seen
    cameras, points = np.where(registered[:, None], rec.cameras, np.nan), np.where(known[:, None], rec.points, np.nan)
    x, args = rec.problem()
    return sfmba.Reconstruction(registered, cameras, points, known, [dict(view=list(map(int, images)))], t, x, args, rec.cam_of,
                                rec.pt_of, rec.obs_feat)


def test_merge_reconstructions_of_two_overlapping_views(be, scene_and_rec):
    """Measured on the MI355X: the similarity against the inverse of the known one at 0.0128 of its bound; points within
    4.3e-16 and centres within 1.2e-15 of the original's, against 9.3e-13, the bound carried through the map; rotations
    within 4.9e-16 against 4.0e-14; 300 of the original's 300 points, one of them from b alone."""
    import sfmba
    scene, rec = scene_and_rec
    reg = np.flatnonzero(rec.registered)
    n = -(-2 * len(reg) // 3)
    A, B0 = view(rec, reg[:n]), view(rec, reg[-n:])
    s0, R0, t0 = 2.7, sr.rodrigues(np.array([0.6, -0.5, 0.62]) * (1.3 / np.linalg.norm([0.6, -0.5, 0.62]))), np.array([5.0, -3.0, 11.0])
    B = B0.transformed(s0, R0, t0)
    assert np.array_equal(np.isnan(B.points), np.isnan(B0.points)) and np.array_equal(np.isnan(B.cameras), np.isnan(B0.cameras))
    merged, est = sfmba.merge_reconstructions(A, B, scene.K, backend=be, seed=1)
    both = A.known & B.known
    assert np.array_equal(merged.registered, A.registered | B.registered) and merged.registered.all()
    assert np.array_equal(merged.known, A.known | B.known) and not (merged.known & ~rec.known).any()
    print(f"{int(merged.known.sum())} of the original's {int(rec.known.sum())} points; {int((B.known & ~A.known).sum())} from b alone")
    assert est.status[0] == est.OK and est.refit_inliers[0] == both.sum() >= 10 and est.refit_mask.all()
    assert merged.rounds[:-1] == A.rounds + B.rounds
    assert merged.rounds[-1] == dict(merged=True, inliers=int(both.sum()), scale=float(est.scale_refit[0]))
    # the recovered similarity inverts the known one, within the bound of the refit's own conditioning
    src, dst = B.points[both], A.points[both]
    want = (1.0 / s0, R0.T, -(R0.T @ t0) / s0)
    got = (est.scale_refit[0], est.R_refit[0], est.t_refit[0])
    ratio = sr.tolerance_ratio(got, want, src, dst)
    ds, dR, dt = sr.estimate_tolerance(src, dst)
    # ... and that bound carried through X = s R X' + t: |ds| |X'| + s dR |X'| + dt, plus the rounding of the two maps
    far = max(np.nanmax(np.linalg.norm(B.points, axis=1)), np.nanmax(np.linalg.norm(B.cameras[:, 3:], axis=1)))
    carried = ds * far + got[0] * dR * far + dt + 32 * EPS * far
    d_pts = np.linalg.norm(merged.points[merged.known] - rec.points[merged.known], axis=1).max()
    d_cen = np.linalg.norm(merged.cameras[:, 3:] - rec.cameras[:, 3:], axis=1).max()
    d_rot = max(np.abs(sr.rodrigues(merged.cameras[i, :3]) - sr.rodrigues(rec.cameras[i, :3])).max() for i in range(len(reg)))
    print(f"similarity / bound {ratio:.4f}; points {d_pts:.3e}, centres {d_cen:.3e} against {carried:.3e}; rotations {d_rot:.3e} "
          f"against {dR + 64 * EPS:.3e}")
    assert 0.0 < ratio <= 1.0 and max(d_pts, d_cen) <= carried and d_rot <= dR + 64 * EPS
    assert np.array_equal(merged.cameras[A.registered], rec.cameras[A.registered])          # where both have one, a's is kept
    assert np.array_equal(merged.points[A.known], rec.points[A.known])
    assert np.isnan(merged.points[~merged.known]).all()
    # the merged problem: observations of the original's, and the original's reprojection error over them
    x, args = merged.problem()
    assert np.isin(merged.obs_feat, rec.obs_feat).all() and len(merged.obs_feat) >= 0.95 * len(rec.obs_feat)
    assert args[0] == len(reg) and args[1] == len(merged.pt_of) and np.array_equal(merged.cam_of, reg)
    x_orig = np.concatenate([rec.cameras[merged.cam_of].ravel(), rec.points[merged.pt_of].ravel()])
    r_merged = sfmba.total_mean_reproj_error(x, args, backend=be)
    r_orig = sfmba.total_mean_reproj_error(x_orig, args, backend=be)
    print(f"reprojection error of the merged problem {r_merged:.12e}, of the original over the same observations {r_orig:.12e}")
    assert abs(r_merged - r_orig) <= 1e-9 * r_orig
    # no solve was run: refine_reconstruction is the caller's next line
    result = sfmba.refine_reconstruction(x, args, rounds=1, backend=be)[0]
    assert result.rmse <= result.rmse0 * (1 + 1e-12)
    # other tracks, too few shared tracks, too few inliers
    with pytest.raises(ValueError, match="fewer than min_inliers"):
        sfmba.merge_reconstructions(A, B, scene.K, min_inliers=int(both.sum()) + 1, backend=be)
    with pytest.raises(ValueError, match="no similarity with min_inliers"):
        sfmba.merge_reconstructions(A, B, scene.K, threshold=1e-18, backend=be)
    import copy
    other = copy.copy(rec.tracks)
    other.feat_track = rec.tracks.feat_track[::-1].copy()
    B.tracks = other
    with pytest.raises(ValueError, match="tracks"):
        sfmba.merge_reconstructions(A, B, scene.K, backend=be)
