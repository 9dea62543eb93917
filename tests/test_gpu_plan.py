"""GPU tests of sfmba_plan_views, sfmba_assemble_problem / sfmba_get_assembled and sfmba_set_keypoints (plan_kernels.hpp)
against the sequential restatement tests/plan_ref.py.

Everything is an integer or a copied double, so every comparison is byte equality: no tolerance anywhere.  The sizes come
from the kernels' own constants: the workgroup, the entries one workgroup scans, and the length from which the wave walks
a track instead of a lane."""
import numpy as np
import pytest

import plan_ref as pr
import track_ref as tr

pytestmark = pytest.mark.gpu

BLOCK, LONG, SCAN = pr.plan_constant("kPlanBlock"), pr.plan_constant("kPlanLong"), pr.plan_constant("kTrackScanItems")


@pytest.fixture(scope="module")
def be():
    import sfmba
    b = sfmba.Backend(0)
    yield b
    b.close()


def views_bytes(v):
    return tuple(getattr(v, name).tobytes() for name in pr.VIEW_FIELDS) + (tuple(v.totals.items()),)


def sub_bytes(s):
    return tuple(getattr(s, name).tobytes() for name in pr.SUB_FIELDS) + (s.points_2d.tobytes(), tuple(s.counts.items()))


def check_views(be, t, cam_reg, trk_known):
    v = be.plan_views(cam_reg, trk_known)
    ref = pr.plan_views_ref(t, cam_reg, trk_known)
    for name in pr.VIEW_FIELDS:
        got = getattr(v, name)
        assert got.dtype == ref[name].dtype and got.shape == ref[name].shape, name
        assert got.tobytes() == ref[name].tobytes(), (name, np.flatnonzero(got != ref[name])[:8])
    assert v.totals == ref["totals"]
    return v


def check_sub(be, t, allpts, cam_use, trk_use, min_views=2):
    s = be.assemble_problem(cam_use, trk_use, min_views=min_views)
    ref = pr.assemble_ref(t, cam_use, trk_use, min_views=min_views, pts=allpts)
    for name in pr.SUB_FIELDS + ("points_2d",):
        got = getattr(s, name)
        assert got.dtype == ref[name].dtype and got.shape == ref[name].shape, name
        assert got.tobytes() == ref[name].tobytes(), (name, np.flatnonzero(np.atleast_1d(got != ref[name]).reshape(len(got), -1).any(axis=1))[:8])
    assert s.counts == ref["counts"]
    assert s.points_2d.tobytes() == allpts[s.obs_feat].tobytes()             # gathered, bit for bit
    return s


def build(be, batch, rng, pair_use=None, **options):
    """Tracks and keypoints of a scene on the device -> (Tracks, all pixels (N, 2))."""
    t = be.build_tracks(*batch, pair_use=pair_use, **options)
    pts = pr.pixels(rng, t.img_ptr)
    be.set_keypoints(pts)
    return t, np.concatenate(pts) if len(pts) else np.empty((0, 2))


def check_masks(be, t, allpts, rng, min_views=(2,)):
    """Both calls over random masks and the masks of all zeros and all ones."""
    n_images, n_tracks = len(t.img_ptr) - 1, t.n_tracks
    zeros_i, ones_i, zeros_t, ones_t = np.zeros(n_images, bool), np.ones(n_images, bool), np.zeros(n_tracks, bool), np.ones(n_tracks, bool)
    ri, rt = rng.random(n_images) < 0.6, rng.random(n_tracks) < 0.5
    for cam, trk in ((ri, rt), (zeros_i, rt), (ones_i, rt), (ri, zeros_t), (ri, ones_t), (ones_i, ones_t)):
        check_views(be, t, cam, trk)
        for mv in min_views:
            check_sub(be, t, allpts, cam, trk, min_views=mv)


# ---- empty inputs ------------------------------------------------------------------------------------------------------
def test_no_tracks(be):
    rng = np.random.default_rng(0)
    ptr = np.array([0, 3, 3, 7], dtype=np.int64)
    for batch, use in (((ptr, [], [0], []), None), ((ptr, [(0, 2)], [0, 2], [(0, 1), (2, 3)]), [0, 0]),
                       ((np.array([0], dtype=np.int64), [], [0], []), None)):
        t, allpts = build(be, batch, rng, pair_use=use)
        n = len(t.img_ptr) - 1
        v = check_views(be, t, np.arange(n) % 2 == 0, [])
        assert v.totals == dict(registered=(n + 1) // 2, known=0, ready=0) and not v.img_tracks.any()
        s = check_sub(be, t, allpts, np.ones(n), [])
        assert s.counts == dict(cameras=0, points=0, observations=0) and s.points_2d.shape == (0, 2)


def test_empty_masks_and_empty_images(be):
    rng = np.random.default_rng(1)
    rows = [0, 0, 40, 0, 55, 30, 0, 61, 0, 0]                    # images with no feature at the start, inside and at the end
    t, allpts = build(be, tr.random_batch(rng, rows, 120), rng, conflicts=1)
    assert t.n_tracks >= 10
    check_masks(be, t, allpts, rng, min_views=(1, 2, 3))
    v = check_views(be, t, np.zeros(10), np.zeros(t.n_tracks))
    assert v.totals == dict(registered=0, known=0, ready=0) and not v.img_gain.any()
    v = check_views(be, t, np.ones(10), np.ones(t.n_tracks))
    assert v.totals == dict(registered=10, known=t.n_tracks, ready=0) and np.array_equal(v.img_known, v.img_tracks)
    assert check_sub(be, t, allpts, np.zeros(10), np.ones(t.n_tracks), min_views=1).n_obs == 0


# ---- track lengths -------------------------------------------------------------------------------------------------------
LENGTHS = sorted({2, LONG - 1, LONG, LONG + 1, 65, 130})


@pytest.mark.parametrize("min_views", [1, 2, 3])
def test_track_lengths_around_the_lane_and_wave_split(be, min_views):
    rng = np.random.default_rng(2)
    sc = tr.Scene(max(LENGTHS))
    for n in LENGTHS + LENGTHS[::-1]:                            # twice: long tracks at both ends of a wave's 64
        sc.path(n)
    t, allpts = build(be, sc.batch(), rng)
    assert sorted(np.diff(t.track_ptr).tolist()) == sorted(LENGTHS + LENGTHS)
    check_masks(be, t, allpts, rng, min_views=(min_views,))
    cam = np.arange(max(LENGTHS)) % 3 != 1                       # a used image pattern that leaves every long track some gaps
    s = check_sub(be, t, allpts, cam, np.ones(t.n_tracks), min_views=min_views)
    assert s.n_points == sum(int(cam[:n].sum()) >= min_views for n in np.diff(t.track_ptr))
    v = check_views(be, t, cam, np.arange(t.n_tracks) % 2)
    assert v.trk_reg_views.tolist() == [int(cam[:n].sum()) for n in np.diff(t.track_ptr)]


# ---- numbers of tracks ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_tracks", [BLOCK - 1, BLOCK, BLOCK + 1, SCAN - 1, SCAN, SCAN + 1, 3 * SCAN + 1])
def test_track_counts_at_the_block_and_scan_edges(be, n_tracks):
    rng = np.random.default_rng(n_tracks)
    per = 6 * n_tracks                                           # sparse: about as many components as pairs
    rows = [0, per, 0, per + 3, per, 0, per + 7, 0]
    batch, use = pr.exact_tracks(rng, rows, 8 * n_tracks // 5, n_tracks)
    t, allpts = build(be, batch, rng, pair_use=use, conflicts=1)
    assert t.n_tracks == n_tracks
    check_masks(be, t, allpts, rng)
    # a trk_use that removes whole scan blocks, and one that leaves a single track per block
    idx = np.arange(n_tracks)
    for trk in ((idx // SCAN) % 2 == 1, idx % SCAN == SCAN - 1, idx >= SCAN, idx < n_tracks - 1):
        check_sub(be, t, allpts, np.ones(len(rows)), trk)
        check_views(be, t, rng.random(len(rows)) < 0.5, trk)


# ---- features per image ---------------------------------------------------------------------------------------------------
def test_image_sizes_at_the_block_edges(be):
    rng = np.random.default_rng(5)
    rows = [BLOCK - 1, BLOCK, BLOCK + 1, 4 * BLOCK + 3, 0, 1]
    t, allpts = build(be, tr.random_batch(rng, rows, 900), rng, conflicts=1)
    check_masks(be, t, allpts, rng, min_views=(1, 2))
    # every feature of every image in a track: all pairwise chains through the largest image
    sc = tr.Scene(4)
    big = [sc.feature(3) for _ in range(rows[3])]
    k = 0
    for image in range(3):
        for _ in range(rows[image]):
            sc.pair(sc.feature(image), big[k])
            k += 1
    t, allpts = build(be, sc.batch(), rng)
    v = check_views(be, t, [1, 0, 1, 0], np.arange(t.n_tracks) % 3 == 0)
    assert v.img_tracks.tolist() == [BLOCK - 1, BLOCK, BLOCK + 1, 3 * BLOCK]
    check_masks(be, t, allpts, rng)


# ---- determinism -----------------------------------------------------------------------------------------------------------
def test_a_second_call_and_another_edge_order_give_the_same_bytes(be):
    rng = np.random.default_rng(9)
    sc = tr.Scene(70)
    for n in (2, LONG + 1, 5, 65, 3):
        sc.path(n)
    sc.star(LONG)
    img_ptr, edges, pair_ptr, pairs = sc.batch()
    extra = tr.random_batch(rng, np.diff(img_ptr), 40, n_edges=12)
    base = (img_ptr, np.concatenate([edges, extra[1]]), np.concatenate([pair_ptr, pair_ptr[-1] + extra[2][1:]]),
            np.concatenate([pairs, extra[3]]))
    t, allpts = build(be, base, rng, conflicts=1)
    cam, trk = rng.random(70) < 0.7, rng.random(t.n_tracks) < 0.7
    want = views_bytes(check_views(be, t, cam, trk)), sub_bytes(check_sub(be, t, allpts, cam, trk))
    assert (views_bytes(be.plan_views(cam, trk)), sub_bytes(be.assemble_problem(cam, trk))) == want
    everything = tr.reorder(base, rng, reverse_edges=True, dup_edges=True, dup_pairs=True, shuffle_edges=True, shuffle_pairs=True)
    t2 = be.build_tracks(*everything, conflicts=1)                # (the same img_ptr: the keypoints stay)
    assert t2.track_feat.tobytes() == t.track_feat.tobytes()
    assert (views_bytes(be.plan_views(cam, trk)), sub_bytes(be.assemble_problem(cam, trk))) == want


# ---- the C interface ---------------------------------------------------------------------------------------------------------
def test_c_interface_refuses_and_reports():
    import ctypes as C
    import sfmba
    from sfmba import _capi
    fresh = sfmba.Backend(0)
    lib = fresh._lib
    try:
        cam, trk = np.array([1, 1], dtype=np.uint8), np.array([1, 1], dtype=np.uint8)
        counts = np.zeros(3, dtype=np.int64)
        # before a build
        assert lib.sfmba_plan_views(fresh._h, 2, _capi.ptr(cam), 2, _capi.ptr(trk), None, None, None, None, None, None, None) == -1
        assert b"sfmba_build_tracks first" in lib.sfmba_last_error(fresh._h)
        assert lib.sfmba_assemble_problem(fresh._h, 2, _capi.ptr(cam), 2, _capi.ptr(trk), None, None, None) == -1
        assert b"sfmba_build_tracks first" in lib.sfmba_last_error(fresh._h)
        assert lib.sfmba_get_assembled(fresh._h, None, None, None, None, None, None) == -1
        assert b"sfmba_build_tracks first" in lib.sfmba_last_error(fresh._h)
        ptr, edges = np.array([0, 2, 5], dtype=np.int64), np.array([[0, 1]], dtype=np.int32)
        pp, pairs = np.array([0, 2], dtype=np.int64), np.array([[0, 1], [1, 2]], dtype=np.int32)
        t = fresh.build_tracks(ptr, edges, pp, pairs)
        assert t.n_tracks == 2
        assert lib.sfmba_get_assembled(fresh._h, None, None, None, None, None, None) == -1       # nothing assembled yet
        assert lib.sfmba_last_error(fresh._h).startswith(b"sfmba_get_assembled:")
        # masks of another length, NULL masks, min_views = 0
        for n_i, n_t, pc, pt in ((3, 2, cam, trk), (2, 1, cam, trk), (2, 2, None, trk), (2, 2, cam, None)):
            a, b = (_capi.ptr(pc) if pc is not None else None), (_capi.ptr(pt) if pt is not None else None)
            assert lib.sfmba_plan_views(fresh._h, n_i, a, n_t, b, None, None, None, None, None, None, None) == -1
            assert lib.sfmba_last_error(fresh._h).startswith(b"sfmba_plan_views:")
            assert lib.sfmba_assemble_problem(fresh._h, n_i, a, n_t, b, None, None, None) == -1
            assert lib.sfmba_last_error(fresh._h).startswith(b"sfmba_assemble_problem:")
        opt = _capi.PlanOptions(0, 0)
        assert lib.sfmba_assemble_problem(fresh._h, 2, _capi.ptr(cam), 2, _capi.ptr(trk), C.byref(opt), _capi.ptr(counts), None) == -1
        assert lib.sfmba_last_error(fresh._h).startswith(b"sfmba_assemble_problem: min_views")
        # NULL options are the defaults; every output may be NULL
        assert lib.sfmba_plan_views(fresh._h, 2, _capi.ptr(cam), 2, _capi.ptr(trk), None, None, None, None, None, None, None) == 0
        assert lib.sfmba_assemble_problem(fresh._h, 2, _capi.ptr(cam), 2, _capi.ptr(trk), None, _capi.ptr(counts), None) == 0
        assert counts.tolist() == [2, 2, 4]
        assert lib.sfmba_get_assembled(fresh._h, None, None, None, None, None, None) == 0
        # points_2d without keypoints, and with keypoints of another img_ptr
        uv = np.empty((4, 2))
        assert lib.sfmba_get_assembled(fresh._h, None, None, None, None, None, _capi.ptr(uv)) == -1
        assert b"sfmba_set_keypoints" in lib.sfmba_last_error(fresh._h) and lib.sfmba_last_error(fresh._h).startswith(b"sfmba_get_assembled:")
        bad = np.array([np.nan, 0.0])
        assert lib.sfmba_set_keypoints(fresh._h, 1, _capi.ptr(np.array([0, 1], dtype=np.int64)), _capi.ptr(bad)) == -1
        assert lib.sfmba_last_error(fresh._h).startswith(b"sfmba_set_keypoints:")
        other = np.array([0, 2, 6], dtype=np.int64)
        px, px_other = np.arange(10, dtype=np.float64), np.arange(12, dtype=np.float64)
        assert lib.sfmba_set_keypoints(fresh._h, 2, _capi.ptr(other), _capi.ptr(px_other)) == 0
        assert lib.sfmba_get_assembled(fresh._h, None, None, None, None, None, _capi.ptr(uv)) == -1
        assert lib.sfmba_last_error(fresh._h).startswith(b"sfmba_get_assembled:")
        assert lib.sfmba_set_keypoints(fresh._h, 2, _capi.ptr(ptr), _capi.ptr(px)) == 0
        of = np.empty(4, dtype=np.int32)
        assert lib.sfmba_get_assembled(fresh._h, None, None, None, None, _capi.ptr(of), _capi.ptr(uv)) == 0
        assert of.tolist() == [0, 3, 1, 4] and uv.tolist() == [[0., 1.], [6., 7.], [2., 3.], [8., 9.]]
        # a build with another img_ptr drops the table and the assembled problem
        fresh.build_tracks(other, edges, pp, pairs)
        assert lib.sfmba_get_assembled(fresh._h, None, None, None, None, None, None) == -1
        assert lib.sfmba_assemble_problem(fresh._h, 2, _capi.ptr(cam), 2, _capi.ptr(trk), None, None, None) == 0
        assert lib.sfmba_get_assembled(fresh._h, None, None, None, None, None, _capi.ptr(uv)) == -1
        assert b"sfmba_set_keypoints" in lib.sfmba_last_error(fresh._h)
        # profile = 1 measures
        fresh.build_tracks(ptr, edges, pp, pairs)
        assert fresh.plan_views(cam, trk, profile=1).kernel_us > 0.0 and fresh.plan_views(cam, trk).kernel_us == 0.0
        assert fresh.assemble_problem(cam, trk, profile=1).kernel_us > 0.0 and fresh.assemble_problem(cam, trk).kernel_us == 0.0
        assert fresh.assemble_problem(cam, trk).points_2d is None                # (the Python side knows the table went)
    finally:
        fresh.close()


# ---- isolation -------------------------------------------------------------------------------------------------------------------
def test_plan_calls_leave_a_problem_its_solve_and_the_tracks_untouched():
    import sfmba
    pb = sfmba.make_problem(8, 120, 900, seed=21)
    rng = np.random.default_rng(17)
    scene = tr.random_batch(rng, [300, 0, 400, SCAN], 700)
    ref = tr.build_tracks_ref(*scene, conflicts=1)
    n_tracks = ref["counts"]["tracks"]
    cam, trk = rng.random(4) < 0.8, rng.random(n_tracks) < 0.6
    pts = pr.pixels(rng, scene[0])

    def solve(with_plan):
        bk = sfmba.Backend(0)
        try:
            if with_plan:
                bk.build_tracks(*scene, conflicts=1)
                bk.set_keypoints(pts)
                bk.plan_views(cam, trk)
                bk.assemble_problem(cam, trk)
            bk.set_problem(*pb.args)
            if with_plan:
                bk.plan_views(cam, trk)
                bk.assemble_problem(cam, trk, min_views=3)
            opt = bk.default_options()
            opt.ftol = 1e-10
            x, res, fun, grad = bk.solve(pb.x0, opt)
            if with_plan:
                bk.plan_views(cam, trk)
                bk.assemble_problem(cam, trk)
                lib = bk._lib
                from sfmba import _capi
                tp = np.empty(n_tracks + 1, dtype=np.int64)
                tf, ti = np.empty(ref["counts"]["observations"], dtype=np.int32), np.empty(ref["counts"]["observations"], dtype=np.int32)
                assert lib.sfmba_get_tracks(bk._h, _capi.ptr(tp), _capi.ptr(tf), _capi.ptr(ti)) == 0
                assert tp.tobytes() == ref["track_ptr"].tobytes() and tf.tobytes() == ref["track_feat"].tobytes()
                assert ti.tobytes() == ref["track_image"].tobytes()
            r = bk.residuals(x)
            return x, np.asarray(fun), np.asarray(grad), r, (res.nfev, res.njev, res.iterations, res.pcg_iterations, res.status)
        finally:
            bk.close()
    xa, fa, ga, ra, ca = solve(False)
    xb, fb, gb, rb, cb = solve(True)
    assert xa.tobytes() == xb.tobytes() and fa.tobytes() == fb.tobytes() and ga.tobytes() == gb.tobytes()
    assert ra.tobytes() == rb.tobytes() and ca == cb
