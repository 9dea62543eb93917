"""GPU tests of sfmba_set_descriptors / sfmba_match_descriptors (k_match, match_kernels.hpp) against the numpy restatement
tests/match_ref.py.

Form A (integer descriptors) is compared bit for bit: the kernel's arithmetic is exact there.  Form B is compared exactly
in idx and good on the queries that are not `contested` (match_ref.contested: a gap below twice the error bound of the
fp32 dot product), and to a relative 1e-12 in dist_sq: the winners' distances are fp64 sums of at most 512 squares of
exactly representable differences, each sum within 512 x 2^-53 of the true value on either side.  Sizes come from the
kernel's own tile constants."""
import numpy as np
import pytest

import match_ref as mr

pytestmark = pytest.mark.gpu

TQ, TT, MR = mr.match_constant("MATCH_TQ"), mr.match_constant("MATCH_TT"), mr.match_constant("MATCH_MFMA_ROWS")
FIELDS = ("query_ptr", "idx", "dist_sq", "good", "edge_good", "edge_status")


@pytest.fixture(scope="module")
def be():
    import sfmba
    b = sfmba.Backend(0)
    yield b
    b.close()


def ints(rng, n, D, dtype=np.uint8):
    return rng.integers(0, 256, size=(n, D)).astype(dtype)


def assert_equal_to_ref(m, descs, edges, ratio=0.5):
    ref = mr.match_batch(descs, edges, ratio)
    for name in FIELDS:
        got = getattr(m, name)
        assert got.dtype == ref[name].dtype and got.shape == ref[name].shape, name
        assert got.tobytes() == ref[name].tobytes(), (name, np.flatnonzero((got != ref[name]).reshape(len(got), -1).any(1))[:8])
    assert m.n_ok == ref["n_ok"]


def run(be, descs, edges, want_form=1, **options):
    assert be.set_descriptors(descs) == want_form
    assert be.form("match_form") == want_form
    return be.match_descriptors(edges, **options)


def pairwise(be, pairs, **options):
    """[(query, train), ...] as one set and one batch -> the matches, compared with the restatement."""
    descs = [a for p in pairs for a in p]
    edges = [(2 * k, 2 * k + 1) for k in range(len(pairs))]
    m = run(be, descs, edges, **options)
    assert_equal_to_ref(m, descs, edges, options.get("ratio", 0.5))
    return m


# ---- form A: every axis swept with the others at their smallest interesting value ----------------------------------------
def test_form_a_query_counts(be):
    rng = np.random.default_rng(1)
    pairwise(be, [(ints(rng, nq, 8), ints(rng, TT + 1, 8)) for nq in (1, TQ - 1, TQ, TQ + 1, 2 * TQ + 3)])


def test_form_a_train_counts(be):
    rng = np.random.default_rng(2)
    counts = sorted({2, 3, MR - 1, MR, MR + 1, TT - 1, TT, TT + 1, 2 * TT + 1})
    pairwise(be, [(ints(rng, MR + 1, 8), ints(rng, nt, 8)) for nt in counts])


@pytest.mark.parametrize("D", [1, 8, 33, 128, 160, 256])
def test_form_a_dimensions(be, D):
    rng = np.random.default_rng(3 + D)
    pairwise(be, [(ints(rng, MR + 1, D), ints(rng, TT + 1, D))])


def test_form_a_mixed_sizes_and_float_input(be):
    rng = np.random.default_rng(4)
    q, t = ints(rng, 2 * TQ + 3, 160), ints(rng, 2 * TT + 1, 160)
    m8 = pairwise(be, [(q, t)])
    mf = pairwise(be, [(q.astype(np.float32), t.astype(np.float32))])          # integer-valued float32: form A as well
    assert mf.idx.tobytes() == m8.idx.tobytes() and mf.dist_sq.tobytes() == m8.dist_sq.tobytes()


def test_form_a_accumulator_limit(be):
    """All values 255 at D = 256: the dot products are 256 x 255^2 = 16646400, just below 2^24."""
    q = np.full((MR + 1, 256), 255, dtype=np.uint8)
    t = np.full((TT + 1, 256), 255, dtype=np.uint8)
    for i in range(len(t)):
        t[i, :i % 7] = 254                                       # d^2 = i mod 7: many exact ties, decided by the index
    m = pairwise(be, [(q, t)])
    assert (m.idx == [0, 7]).all() and (m.dist_sq == 0).all() and not m.good.any()


# ---- planted neighbours ------------------------------------------------------------------------------------------------
def plant(rng, nt, D, first, second, d1=1, d2=9):
    """A query and a train image of random rows (d^2 about D x 10^4) with a row at d^2 = d1 at `first` and one at
    d^2 = d2 at `second` (d1, d2 sums of squares placed on separate coordinates)."""
    q = ints(rng, 3, D)
    q[:, :4] = 100
    t = ints(rng, nt, D)

    def at(dsq):
        row = q[1].astype(np.int64).copy()
        k = 0
        while dsq > 0:
            s = int(np.sqrt(dsq))
            row[k] += s
            dsq -= s * s
            k += 1
        return row.astype(np.uint8)
    t[first], t[second] = at(d1), at(d2)
    return q, t


def test_planted_neighbours_at_every_position(be):
    rng = np.random.default_rng(5)
    nt = 2 * TT + 5                                              # a ragged last tile of five rows
    places = [(0, nt - 1), (nt - 1, 0), (3, 40), (TT - 1, TT), (TT, TT - 1), (1, 5), (5, 1), (MR - 1, MR),
              (2 * TT + 1, 2 * TT + 4), (2 * TT + 4, 2 * TT)]
    pairs = [plant(rng, nt, 128, a, b) for a, b in places]
    m = pairwise(be, pairs)
    for k, (a, b) in enumerate(places):
        o = int(m.query_ptr[k]) + 1
        assert tuple(m.idx[o]) == (a, b) and tuple(m.dist_sq[o]) == (1.0, 9.0) and m.good[o]


def test_exact_ties_prefer_the_lower_index(be):
    rng = np.random.default_rng(6)
    nt = 2 * TT + 5
    pairs, want = [], []
    for i, j in ((2, 6), (5, TT + 2), (1, 3), (TT - 1, 2 * TT + 4)):       # across half-waves, tiles, inside one lane
        q, t = plant(rng, nt, 128, i, j, d1=1, d2=1)                         # the duplicate is the nearest
        assert (t[i] == t[j]).all()
        pairs.append((q, t)); want.append(((i, j), (1.0, 1.0)))
        q, t = plant(rng, nt, 128, i, j, d1=4, d2=4)                         # ... is the second nearest
        t[7] = q[1]                                                           # a query equal to a train row: d1^2 = 0
        pairs.append((q, t)); want.append(((7, i), (0.0, 4.0)))
    m = pairwise(be, pairs)
    for k, (idx, dist) in enumerate(want):
        o = int(m.query_ptr[k]) + 1
        assert tuple(m.idx[o]) == idx and tuple(m.dist_sq[o]) == dist


def test_ratio_boundary_is_strict(be):
    rng = np.random.default_rng(7)
    m = pairwise(be, [plant(rng, TT + 1, 128, 9, 2, d1=1, d2=4), plant(rng, TT + 1, 128, 9, 2, d1=1, d2=5)])
    a, b = int(m.query_ptr[0]) + 1, int(m.query_ptr[1]) + 1
    assert tuple(m.dist_sq[a]) == (1.0, 4.0) and not m.good[a]              # 1 < 0.25 x 4 is false
    assert tuple(m.dist_sq[b]) == (1.0, 5.0) and m.good[b]
    # another ratio moves the boundary: 0.6^2 x 4 = 1.44 > 1
    m = pairwise(be, [plant(rng, TT + 1, 128, 9, 2, d1=1, d2=4)], ratio=0.6)
    assert m.good[1]


# ---- a mixed batch ------------------------------------------------------------------------------------------------------
def test_mixed_batch_equals_every_edge_alone(be):
    rng = np.random.default_rng(8)
    sizes = [TQ + 5, 0, 1, 2 * TT + 1, 3, MR]
    descs = [ints(rng, n, 33) for n in sizes]
    edges = [(0, 3), (3, 0), (0, 3), (3, 3), (0, 1), (1, 0), (0, 2), (2, 0), (4, 5), (5, 4), (2, 4)]
    m = run(be, descs, edges)
    assert_equal_to_ref(m, descs, edges)
    assert list(m.edge_status) == [0, 0, 0, 0, 1, 1, 1, 0, 0, 0, 0]
    assert (m.idx[int(m.query_ptr[3]):int(m.query_ptr[4]), 0] == np.arange(sizes[3])).all()       # u == v: itself first
    for e, edge in enumerate(edges):
        alone = be.match_descriptors([edge])
        sl = slice(int(m.query_ptr[e]), int(m.query_ptr[e + 1]))
        assert alone.idx.tobytes() == m.idx[sl].tobytes() and alone.dist_sq.tobytes() == m.dist_sq[sl].tobytes(), e
        assert alone.good.tobytes() == m.good[sl].tobytes() and alone.edge_good[0] == m.edge_good[e], e
        assert alone.edge_status[0] == m.edge_status[e], e
        assert np.array_equal(m.pairs(e), mr.good_pairs(descs[edge[0]], descs[edge[1]])), e
    none = be.match_descriptors(np.empty((0, 2), dtype=np.int32))
    assert none.n_ok == 0 and none.idx.shape == (0, 2) and list(none.query_ptr) == [0]


# ---- which form ---------------------------------------------------------------------------------------------------------
def test_form_decision(be):
    rng = np.random.default_rng(9)
    q, t = ints(rng, MR + 1, 33), ints(rng, TT + 1, 33)
    ref = mr.match_batch([q, t], [(0, 1)])
    a = run(be, [q, t], [(0, 1)], want_form=1)
    run(be, [q.astype(np.float32), t.astype(np.float32)], [(0, 1)], want_form=1)
    b = run(be, [q, t], [(0, 1)], want_form=1, form=2)                         # B forced on integer data: the same result
    for name in ("idx", "dist_sq", "good"):
        assert getattr(a, name).tobytes() == ref[name].tobytes() == getattr(b, name).tobytes(), name
    for bad in (0.5, 256.0, -1.0):
        tf = t.astype(np.float32)
        tf[TT, 32] = bad                                         # the very last value of the set
        m = run(be, [q.astype(np.float32), tf], [(0, 1)], want_form=2)
        assert m.edge_status[0] == 0
        with pytest.raises(ValueError, match="form A"):
            be.match_descriptors([(0, 1)], form=1)
    wide = [ints(rng, 3, 257), ints(rng, 4, 257)]                # wider than form A's row
    assert be.set_descriptors(wide) == 2
    with pytest.raises(ValueError):
        be.match_descriptors([(0, 2)])                           # an image id out of range
    with pytest.raises(ValueError):
        be.match_descriptors([(0, 1)], ratio=float("nan"))
    with pytest.raises(ValueError):
        be.match_descriptors([(0, 1)], ratio=0.0)


def test_calls_before_set_descriptors_fail():
    import sfmba
    b = sfmba.Backend(0)
    try:
        with pytest.raises(ValueError):
            b.match_descriptors([(0, 1)])
        with pytest.raises(ValueError, match="no descriptors"):
            b.form("match_form")
    finally:
        b.close()


# ---- form B -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def form_b_cases():
    out = []
    for D, nq, nt in mr.FORM_B_SHAPES:
        q, t = mr.form_b_fixture(D, nq, nt)
        out.append((q, t, mr.match_edge(q, t), mr.contested(q, t)))
    return out


@pytest.mark.parametrize("k", range(len(mr.FORM_B_SHAPES)))
def test_form_b_against_fp64(be, form_b_cases, k):
    q, t, ref, skip = form_b_cases[k]
    assert skip.mean() <= mr.CONTESTED_CAP
    m = run(be, [q, t], [(0, 1)], want_form=2)
    keep = ~skip
    assert np.array_equal(m.idx[keep], ref["idx"][keep][:, :2])
    assert np.array_equal(m.good[keep], ref["good"][keep])
    assert 0.3 < m.good.mean() < 0.7                             # about half pass the ratio test
    assert np.all(np.abs(m.dist_sq[keep] - ref["dist_sq"][keep]) <= 1e-12 * ref["dist_sq"][keep])
    assert m.edge_good[0] == int(m.good.sum()) and m.edge_status[0] == 0
    again = be.match_descriptors([(0, 1)])
    assert again.idx.tobytes() == m.idx.tobytes() and again.dist_sq.tobytes() == m.dist_sq.tobytes()


def test_form_b_non_finite_rows_are_never_neighbours(be, form_b_cases):
    q, t, _, _ = form_b_cases[1]
    t = t.copy()
    t[5, 3] = np.nan
    t[TT + 1, 0] = np.inf
    t[7] = q[0]                                                  # (the rows next to them still are)
    ref = mr.match_edge(q, t)
    skip = mr.contested(q, t)
    two = np.stack([t[5], t[9]])                                 # a train image of two rows, one of them not finite
    inf_q = np.concatenate([q[:3], np.full((1, q.shape[1]), np.inf, dtype=np.float32)])
    m = run(be, [q, t, two, inf_q], [(0, 1), (0, 2), (3, 1)], want_form=2)
    a = slice(0, len(q))
    assert not np.isin(m.idx[a], (5, TT + 1)).any()
    assert np.array_equal(m.idx[a][~skip], ref["idx"][~skip]) and np.array_equal(m.good[a][~skip], ref["good"][~skip])
    assert m.idx[0, 0] == 7 and m.dist_sq[0, 0] == 0.0
    b = slice(len(q), 2 * len(q))
    assert (m.idx[b, 0] == 1).all() and (m.idx[b, 1] == -1).all() and not m.good[b].any()
    assert np.isfinite(m.dist_sq[b, 0]).all() and np.isinf(m.dist_sq[b, 1]).all()
    last = int(m.query_ptr[3]) - 1                               # a query that is not finite has no neighbour at all
    assert tuple(m.idx[last]) == (-1, -1) and not m.good[last] and m.edge_status[2] == 0


# ---- the whole of _match_features -------------------------------------------------------------------------------------
def test_match_features_end_to_end(be):
    import sfmba
    from sfmba.synthetic import K_SCEAUX as K
    rng = np.random.default_rng(11)
    X = np.column_stack([rng.uniform(-2, 2, 80), rng.uniform(-1.5, 1.5, 80), rng.uniform(6, 10, 80)])
    point_desc = ints(rng, 80, 128)

    def rot_y(a):
        return np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    poses = [(np.eye(3), np.zeros(3)), (rot_y(0.08), np.array([-0.8, 0.05, 0.1])), (rot_y(-0.1), np.array([0.9, -0.1, 0.05]))]
    seen = [np.arange(80), np.arange(60), np.arange(50, 80)]
    descs, pts = [], []
    for (R, t), vis in zip(poses, seen):
        vis = rng.permutation(vis)
        x = (K @ (R @ X[vis].T + t[:, None])).T
        px = x[:, :2] / x[:, 2:]
        px[:5] = rng.uniform(0, 2000, (5, 2))                    # five right descriptors at wrong pixels
        descs.append(np.concatenate([point_desc[vis], ints(rng, 20, 128)]))
        pts.append(np.concatenate([px, rng.uniform(0, 2000, (20, 2))]))
    got = sfmba.match_features(descs, pts, K, min_matches=15, seed=3, backend=be)
    want = []
    for u in range(3):
        for v in range(3):
            if u <= v:
                continue
            gp = mr.good_pairs(descs[u], descs[v])
            if len(gp) <= 8:
                continue
            F, mask = sfmba.find_fundamental_mat(pts[u][gp[:, 0]], pts[v][gp[:, 1]], seed=3, backend=be)
            inl = gp[mask.ravel() > 0]
            if len(inl) > 15:
                want.append((u, v, inl))
    assert [(u, v) for u, v, *_ in got] == [(u, v) for u, v, _ in want] == [(1, 0), (2, 0)]
    for (u, v, inl, F, E), (_, _, inl_ref) in zip(got, want):
        assert np.array_equal(inl, inl_ref)
        assert np.allclose(E, K.T @ F @ K) and abs(np.linalg.norm(F) - 1.0) < 1e-12
    knn = sfmba.knn_match(descs[1], descs[0], backend=be)
    ref = mr.match_edge(descs[1], descs[0])
    assert len(knn) == len(descs[1]) and all(len(pair) == 2 for pair in knn)
    assert [[n.trainIdx for n in pair] for pair in knn] == ref["idx"].tolist()
    assert knn[3][1].queryIdx == 3 and knn[3][1].distance == np.float32(np.sqrt(ref["dist_sq"][3, 1]))


# ---- other checks -----------------------------------------------------------------------------------------------------
def test_kernel_time_only_with_profile(be):
    rng = np.random.default_rng(12)
    be.set_descriptors([ints(rng, TQ, 128), ints(rng, 2 * TT, 128)])
    assert be.match_descriptors([(0, 1)], profile=1).kernel_us > 0.0
    assert be.match_descriptors([(0, 1)]).kernel_us == 0.0


def test_matching_leaves_a_set_problem_untouched():
    import sfmba
    rng = np.random.default_rng(13)
    descs = [ints(rng, TQ + 1, 128), rng.standard_normal((TT + 1, 128)).astype(np.float32)]
    pb = sfmba.make_problem(8, 120, 900, seed=21)

    def solve(match):
        bk = sfmba.Backend(0)
        try:
            if match:
                bk.set_descriptors(descs[:1])                    # before any problem exists
                bk.match_descriptors([(0, 0)])
            bk.set_problem(*pb.args)
            if match:
                bk.set_descriptors(descs)
                bk.match_descriptors([(0, 1), (1, 0)], form=2)
            opt = bk.default_options()
            opt.ftol = 1e-10
            x, res, _, _ = bk.solve(pb.x0, opt, want_fun=False, want_grad=False)
            if match:
                bk.match_descriptors([(1, 1)])
                r = bk.residuals(x)
            else:
                r = bk.residuals(x)
            return x, r, res.nfev
        finally:
            bk.close()
    xa, ra, na = solve(False)
    xb, rb, nb = solve(True)
    assert xa.tobytes() == xb.tobytes() and ra.tobytes() == rb.tobytes() and na == nb
