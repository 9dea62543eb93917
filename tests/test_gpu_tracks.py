"""GPU tests of sfmba_build_tracks / sfmba_get_tracks (track_kernels.hpp) against the sequential restatement
tests/track_ref.py.

Everything is integers, so every comparison is byte equality of feat_track, track_ptr, track_feat, track_image and the
counts: no tolerance anywhere.  The sizes come from the kernels' own constants: the workgroup, the entries one workgroup
scans, and the length from which the wave sorts a component instead of a lane."""
import json
import os

import numpy as np
import pytest

import track_ref as tr
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

BLOCK, SCAN, LONG = tr.track_constant("kTrackBlock"), tr.track_constant("kTrackScanItems"), tr.track_constant("kTrackLong")


@pytest.fixture(scope="module")
def be():
    import sfmba
    b = sfmba.Backend(0)
    yield b
    b.close()


def as_bytes(t):
    return tuple(getattr(t, name).tobytes() for name in tr.FIELDS) + (tuple(t.counts[k] for k in tr.COUNTS),)


def check(be, batch, pair_use=None, **options):
    """One build compared with the restatement, entry for entry -> the Tracks."""
    t = be.build_tracks(*batch, pair_use=pair_use, **options)
    ref = tr.build_tracks_ref(*batch, pair_use=pair_use, **{k: v for k, v in options.items() if k != "profile"})
    for name in tr.FIELDS:
        got = getattr(t, name)
        assert got.dtype == ref[name].dtype and got.shape == ref[name].shape, name
        assert got.tobytes() == ref[name].tobytes(), (name, np.flatnonzero(got != ref[name])[:8])
    assert t.counts == ref["counts"]
    assert t.n_tracks == ref["counts"]["tracks"]
    return t


# ---- empty inputs ------------------------------------------------------------------------------------------------------
def test_empty_inputs(be):
    ptr = np.array([0, 3, 3, 7], dtype=np.int64)
    for batch, use in (((ptr, [], [0], []), None), ((ptr, [(0, 2), (2, 0)], [0, 0, 0], []), None),
                       ((ptr, [(0, 2)], [0, 2], [(0, 1), (2, 3)]), [0, 0]), ((np.array([0], dtype=np.int64), [], [0], []), None)):
        t = check(be, batch, pair_use=use)
        assert t.n_tracks == 0 and np.all(t.feat_track == t.UNMATCHED) and t.track_ptr.tolist() == [0]
    t = check(be, (ptr, [(2, 0)], [0, 1], [(3, 1)]))
    assert t.feat_track.tolist() == [-1, 0, -1, -1, -1, -1, 0] and t.track_feat.tolist() == [1, 6]


# ---- component sizes -----------------------------------------------------------------------------------------------------
SIZES = sorted({2, 3, LONG - 1, LONG, LONG + 1, 64, 65, 130})


@pytest.mark.parametrize("shape", ["star", "path", "path_descending"])
def test_component_sizes(be, shape):
    sc = tr.Scene(max(SIZES))
    for n in SIZES:
        if shape == "star":
            sc.star(n)
        else:
            sc.path(n, descending=shape == "path_descending")
    t = check(be, sc.batch())
    assert np.diff(t.track_ptr).tolist() == SIZES and t.counts["conflict"] == 0


def test_very_long_path_over_three_images(be):
    sc = tr.Scene(3)
    sc.path(4097, period=3, descending=True)
    batch = sc.batch()
    kept = check(be, batch, conflicts=1)
    assert kept.n_tracks == 1 and np.array_equal(kept.track_feat, np.arange(4097))
    dropped = check(be, batch)
    assert np.all(dropped.feat_track == dropped.CONFLICT) and dropped.counts["conflict"] == 1


# ---- conflicts -------------------------------------------------------------------------------------------------------------
def test_conflicts(be):
    sc = tr.Scene(6)
    a0, a1 = sc.feature(0), sc.feature(0)
    b = sc.feature(1)
    sc.pair(a0, b); sc.pair(b, a1)                               # two features of image 0 through image 1
    c0 = sc.feature(2)
    chain = [sc.feature(k) for k in (3, 4, 5, 1)] + [sc.feature(2)]
    sc.pair(c0, chain[0])
    for x, y in zip(chain, chain[1:]):
        sc.pair(x, y)                                            # two features of image 2 through a chain of four
    sc.star(4, first_image=1)                                    # a clean component next to them
    d0, d1 = sc.feature(4), sc.feature(5)
    e0 = sc.feature(4)
    sc.pair(d0, d1); sc.pair(d1, e0)                             # three features, two of image 4: short for 4 and conflicting
    batch = sc.batch()
    t = check(be, batch)
    assert t.n_tracks == 1 and t.counts["conflict"] == 3
    t = check(be, batch, min_length=4)
    assert t.counts == dict(components=4, tracks=1, short=0, long=0, conflict=3, observations=4)
    t = check(be, batch, min_length=4, conflicts=1)
    assert t.counts["short"] == 2 and t.counts["tracks"] == 2
    # short AND conflicting: a conflict takes three features (a pair joins two images), so min_length is 4 here
    sc2 = tr.Scene(2)
    p, q, r = sc2.feature(0), sc2.feature(1), sc2.feature(0)
    sc2.pair(p, q); sc2.pair(q, r)
    t = check(be, sc2.batch(), min_length=4)
    assert t.feat_track.tolist() == [-3, -3, -3]
    t = check(be, sc2.batch(), min_length=3, max_length=3, conflicts=1)
    assert t.feat_track.tolist() == [0, 0, 0]


# ---- length options --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("options", [dict(min_length=1), dict(min_length=2), dict(min_length=3), dict(max_length=5),
                                     dict(max_length=4), dict(max_length=6), dict(min_length=5, max_length=5)],
                         ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()))
def test_length_options(be, options):
    sc = tr.Scene(8)
    for n in (2, 5, 3, 8, 5, 2):
        sc.path(n)
    check(be, sc.batch(), **options)


# ---- boundaries --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [BLOCK - 1, BLOCK, BLOCK + 1, SCAN - 1, SCAN, SCAN + 1, 3 * SCAN + 1])
def test_feature_counts_at_the_block_and_scan_edges(be, N):
    rng = np.random.default_rng(N)
    rows = [0, N // 3, 0, N // 3, N - 2 * (N // 3) - 7, 0, 7, 0]    # empty images at the start, inside and at the end
    batch = tr.random_batch(rng, rows, N // 2)
    assert batch[0][-1] == N
    check(be, batch)
    check(be, batch, conflicts=1, min_length=3)


@pytest.mark.parametrize("M", [BLOCK - 1, BLOCK, BLOCK + 1, SCAN - 1, SCAN, SCAN + 1])
def test_pair_counts_at_the_block_and_scan_edges(be, M):
    rng = np.random.default_rng(100 + M)
    batch = tr.random_batch(rng, [SCAN, 0, SCAN + 3, 5 * BLOCK], M)
    assert len(batch[3]) == M
    check(be, batch)
    check(be, batch, conflicts=1)


def test_more_components_than_one_scan_block(be):
    n = SCAN + BLOCK + 1                                         # so many components of two: the second scan has two levels too
    ptr = np.array([0, n, 2 * n + 5], dtype=np.int64)
    rng = np.random.default_rng(5)
    pairs = np.stack([np.arange(n), rng.permutation(n)], axis=1).astype(np.int32)
    t = check(be, (ptr, [(0, 1)], [0, n], pairs), pair_use=(np.arange(n) % 7 != 3))
    assert t.n_tracks == n - len(range(3, n, 7))


# ---- invariance ----------------------------------------------------------------------------------------------------------------
def test_the_order_of_edges_and_pairs_does_not_show(be):
    rng = np.random.default_rng(9)
    sc = tr.Scene(70)
    for n in (2, LONG + 1, 5, 65, 3):
        sc.path(n)
    sc.star(LONG)
    img_ptr, edges, pair_ptr, pairs = sc.batch()
    extra = tr.random_batch(rng, np.diff(img_ptr), 40, n_edges=12)
    base = (img_ptr, np.concatenate([edges, extra[1]]), np.concatenate([pair_ptr, pair_ptr[-1] + extra[2][1:]]),
            np.concatenate([pairs, extra[3]]))
    for conflicts in (0, 1):
        want = as_bytes(check(be, base, conflicts=conflicts))
        for how in ("reverse_edges", "dup_edges", "dup_pairs", "shuffle_edges", "shuffle_pairs"):
            assert as_bytes(be.build_tracks(*tr.reorder(base, rng, **{how: True}), conflicts=conflicts)) == want, how
        everything = tr.reorder(base, rng, reverse_edges=True, dup_edges=True, dup_pairs=True, shuffle_edges=True, shuffle_pairs=True)
        assert as_bytes(be.build_tracks(*everything, conflicts=conflicts)) == want
        assert as_bytes(be.build_tracks(*base, conflicts=conflicts)) == want         # and a second call


def test_masking_a_pair_equals_removing_it(be):
    rng = np.random.default_rng(11)
    batch = tr.random_batch(rng, [40, 50, 0, 60], 90)
    img_ptr, edges, pair_ptr, pairs = batch
    use = rng.random(len(pairs)) < 0.6
    masked = check(be, batch, pair_use=use, conflicts=1)
    edge_of = np.repeat(np.arange(len(edges)), np.diff(pair_ptr))
    half = use | (rng.random(len(pairs)) < 0.5)                  # some of the unused pairs removed, the rest masked
    ptr2 = np.searchsorted(edge_of[half], np.arange(len(edges) + 1)).astype(np.int64)
    assert as_bytes(be.build_tracks(img_ptr, edges, ptr2, pairs[half], pair_use=use[half], conflicts=1)) == as_bytes(masked)
    ptr3 = np.searchsorted(edge_of[use], np.arange(len(edges) + 1)).astype(np.int64)
    assert as_bytes(be.build_tracks(img_ptr, edges, ptr3, pairs[use], conflicts=1)) == as_bytes(masked)


# ---- the C interface ---------------------------------------------------------------------------------------------------------
def test_c_interface_refuses_and_reports(be):
    import ctypes as C
    from sfmba import _capi
    lib = be._lib
    import sfmba
    fresh = sfmba.Backend(0)
    try:
        assert lib.sfmba_get_tracks(fresh._h, None, None, None) == -1
        assert b"sfmba_build_tracks first" in lib.sfmba_last_error(fresh._h)
        ptr, edges = np.array([0, 2, 5], dtype=np.int64), np.array([[0, 1]], dtype=np.int32)
        pp, pairs = np.array([0, 2], dtype=np.int64), np.array([[0, 1], [1, 2]], dtype=np.int32)
        for bad in (dict(pairs=np.array([[0, 1], [2, 3]], dtype=np.int32)), dict(edges=np.array([[1, 1]], dtype=np.int32)),
                    dict(edges=np.array([[0, 2]], dtype=np.int32)), dict(ptr=np.array([0, 6, 5], dtype=np.int64)),
                    dict(pp=np.array([1, 2], dtype=np.int64)), dict(min_length=0), dict(min_length=3, max_length=2)):
            a = dict(ptr=ptr, edges=edges, pp=pp, pairs=pairs, min_length=2, max_length=0)
            a.update(bad)
            opt = _capi.TrackOptions(a["min_length"], a["max_length"], 0, 0)
            rc = lib.sfmba_build_tracks(fresh._h, 2, _capi.ptr(a["ptr"]), 1, _capi.ptr(a["edges"]), _capi.ptr(a["pp"]),
                                        _capi.ptr(a["pairs"]), None, C.byref(opt), None, None, None)
            assert rc == -1 and lib.sfmba_last_error(fresh._h).startswith(b"sfmba_build_tracks:"), bad
        # NULL options are the defaults; every output may be NULL; profile = 1 measures
        assert lib.sfmba_build_tracks(fresh._h, 2, _capi.ptr(ptr), 1, _capi.ptr(edges), _capi.ptr(pp), _capi.ptr(pairs), None, None,
                                      None, None, None) == 0
        tp, tf, ti = np.empty(3, dtype=np.int64), np.empty(4, dtype=np.int32), np.empty(4, dtype=np.int32)
        assert lib.sfmba_get_tracks(fresh._h, _capi.ptr(tp), _capi.ptr(tf), _capi.ptr(ti)) == 0
        assert tp.tolist() == [0, 2, 4] and tf.tolist() == [0, 3, 1, 4] and ti.tolist() == [0, 1, 0, 1]
        t = fresh.build_tracks(ptr, edges, pp, pairs, profile=1)
        assert t.kernel_us > 0.0 and fresh.build_tracks(ptr, edges, pp, pairs).kernel_us == 0.0
    finally:
        fresh.close()


# ---- isolation -------------------------------------------------------------------------------------------------------------------
def test_tracks_leave_a_problem_and_its_solve_untouched():
    import sfmba
    pb = sfmba.make_problem(8, 120, 900, seed=21)
    rng = np.random.default_rng(17)
    first = tr.random_batch(rng, [30, 40, 50], 60)
    second = tr.random_batch(rng, [300, 0, 400, SCAN], 700)

    def solve(with_tracks):
        bk = sfmba.Backend(0)
        try:
            if with_tracks:
                bk.build_tracks(*first)                          # before any problem exists
            bk.set_problem(*pb.args)
            if with_tracks:
                bk.build_tracks(*second, conflicts=1)
            opt = bk.default_options()
            opt.ftol = 1e-10
            x, res, fun, grad = bk.solve(pb.x0, opt)
            if with_tracks:
                t = bk.build_tracks(*first)
                ref = tr.build_tracks_ref(*first)                # the second build's set is what get_tracks hands out
                assert t.track_feat.tobytes() == ref["track_feat"].tobytes() and t.track_ptr.tobytes() == ref["track_ptr"].tobytes()
            r = bk.residuals(x)
            return x, np.asarray(fun), np.asarray(grad), r, (res.nfev, res.njev, res.iterations, res.pcg_iterations, res.status)
        finally:
            bk.close()
    xa, fa, ga, ra, ca = solve(False)
    xb, fb, gb, rb, cb = solve(True)
    assert xa.tobytes() == xb.tobytes() and fa.tobytes() == fb.tobytes() and ga.tobytes() == gb.tobytes()
    assert ra.tobytes() == rb.tobytes() and ca == cb


# ---- through the layers ------------------------------------------------------------------------------------------------------------
def test_matches_to_problem_to_triangulation(be):
    import sfmba
    pb = sfmba.make_problem(6, 60, 400, seed=4)
    C, P = pb.n_cameras, pb.n_points
    ci, pi, uv = np.asarray(pb.camera_indices), np.asarray(pb.point_indices), np.asarray(pb.points_2d, dtype=np.float64)
    # ground truth: one observation per (point, camera), the first; as per-image feature lists in a shuffled row order
    _, firsts = np.unique(pi * C + ci, return_index=True)
    firsts.sort()
    ci, pi, uv = ci[firsts], pi[firsts], uv[firsts]
    rng = np.random.default_rng(8)
    feats = [rng.permutation(np.flatnonzero(ci == c)) for c in range(C)]           # image c: its observations, row by row
    row_of = np.empty(len(ci), dtype=np.int64)
    for f in feats:
        row_of[f] = np.arange(len(f))
    pts = [uv[f] for f in feats]
    # every track chained through its consecutive cameras: no edge sees a whole track of three or more
    pair_lists = {}
    for p in range(P):
        obs = np.flatnonzero(pi == p)
        obs = obs[np.argsort(ci[obs])]
        for a, b in zip(obs, obs[1:]):
            pair_lists.setdefault((int(ci[b]), int(ci[a])), []).append((row_of[b], row_of[a]))
    matches = [(u, v, np.array(pr)) for (u, v), pr in pair_lists.items()]
    t = sfmba.build_tracks(matches, [len(f) for f in feats], backend=be)
    n_points, cam2, pt2, uv2 = t.problem(pts)
    # the points seen twice or more, renumbered by their first feature
    views = np.bincount(pi, minlength=P)
    seen = np.flatnonzero(views >= 2)
    img_ptr = t.img_ptr
    gid = img_ptr[ci] + row_of
    first_feat = np.array([gid[pi == p].min() for p in seen])
    order = seen[np.argsort(first_feat)]                          # track k is original point order[k]
    assert n_points == len(seen) and t.counts["conflict"] == 0
    want_obs = np.concatenate([np.flatnonzero(pi == p)[np.argsort(gid[pi == p])] for p in order])
    assert np.array_equal(cam2, ci[want_obs]) and np.array_equal(order[pt2], pi[want_obs]) and np.array_equal(uv2, uv[want_obs])
    assert np.all(t.feat_track[gid[np.isin(pi, np.flatnonzero(views < 2))]] == t.UNMATCHED)
    # triangulated at the true cameras: the same points as on the original problem, within the recorded bound of the
    # linear stage (the two differ in the order of a track's rows only)
    bound = json.load(open(os.path.join(GOLDEN, "triangulate_bounds.json")))["problem"]["bound_rel"]
    be.set_precision(64)
    be.set_problem(C, P, ci, pi, uv, pb.K)
    a = be.triangulate(pb.x_true, max_iter=0, min_angle_deg=2.0, min_depth=-np.inf)
    x2 = np.concatenate([pb.x_true[:6 * C], pb.x_true[6 * C:].reshape(P, 3)[order].ravel()])
    be.set_problem(C, n_points, cam2, pt2, uv2, pb.K)
    b = be.triangulate(x2, max_iter=0, min_angle_deg=2.0, min_depth=-np.inf)
    assert np.array_equal(a.status[order], b.status) and np.array_equal(a.views[order], b.views)
    ok = np.flatnonzero(b.status == b.OK)
    assert len(ok) >= 0.9 * n_points
    Xa, Xb = a.points[order][ok], b.points[ok]
    worst = float((np.abs(Xa - Xb).max(axis=1) / np.maximum(1.0, np.abs(Xa).max(axis=1))).max())
    print(f"triangulated from built tracks vs from the original problem over {len(ok)} tracks: {worst:.3e} (bound {bound:.3e})")
    assert worst <= bound
