"""Host-side tests of feature tracks: the restatement tests/track_ref.py against an independent yardstick, the Python
argument checks, `Tracks.problem`, and the C++ argument checks (csrc/track_inputs.hpp) as a stand-alone program under
AddressSanitizer + UndefinedBehaviorSanitizer.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import track_ref as tr
from conftest import ROOT

PKG = os.path.join(ROOT, "sfm-python_amd")


def random_case(seed):
    rng = np.random.default_rng(seed)
    n_images = int(rng.integers(2, 9))
    rows = rng.integers(0, 12, n_images)
    rows[rng.integers(0, n_images)] += 1
    rows[(np.argmax(rows) + 1) % n_images] += 1                  # two images with rows at the least
    return tr.random_batch(rng, rows, int(rng.integers(0, 40)))


def test_restatement_partition_equals_scipy_connected_components():
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    for seed in range(200):
        img_ptr, edges, pair_ptr, pairs = random_case(seed)
        N = int(img_ptr[-1])
        g = tr.global_pairs(img_ptr, edges, pair_ptr, pairs)
        label, used = tr.components_ref(N, g)
        _, lab = connected_components(coo_matrix((np.ones(len(g)), (g[:, 0], g[:, 1])), shape=(N, N)), directed=False)
        smallest = np.full(lab.max() + 1 if N else 0, N, dtype=np.int64)
        np.minimum.at(smallest, lab, np.arange(N))               # canonical: a component's smallest member
        assert np.array_equal(smallest[lab], label), seed
        assert np.array_equal(used, np.isin(np.arange(N), g)), seed
        # and the interface's outputs say the same partition
        ref = tr.build_tracks_ref(img_ptr, edges, pair_ptr, pairs, conflicts=1)
        ft = ref["feat_track"]
        assert np.array_equal(ft >= 0, used), seed
        first = ref["track_feat"][ref["track_ptr"][:-1]]
        assert np.all(np.diff(first) > 0) and np.array_equal(first[ft[used]], label[used]), seed


def test_every_one_hop_set_lies_inside_its_component():
    for seed in range(50):
        batch = random_case(1000 + seed)
        label, _ = tr.components_ref(int(batch[0][-1]), tr.global_pairs(*batch))
        hops = tr.one_hop_sets(*batch)
        assert hops or batch[2][-1] == 0
        for f, others in hops.items():
            assert all(label[o] == label[f] for o in others), (seed, f)


def test_restatement_on_a_hand_written_example():
    # image 0: rows a0 a1; image 1: rows b0 b1 b2; image 2: row c0.  a0-b0, b0-c0 (a clean track of three); a1-b1,
    # a1-b2 (two features of image 1: a conflict); nothing else
    img_ptr, edges = [0, 2, 5, 6], [(0, 1), (1, 2)]
    pair_ptr, pairs = [0, 3, 4], [(0, 0), (1, 1), (1, 2), (0, 0)]
    ref = tr.build_tracks_ref(img_ptr, edges, pair_ptr, pairs)
    assert ref["feat_track"].tolist() == [0, -3, 0, -3, -3, 0]
    assert ref["track_ptr"].tolist() == [0, 3] and ref["track_feat"].tolist() == [0, 2, 5] and ref["track_image"].tolist() == [0, 1, 2]
    assert ref["counts"] == dict(components=2, tracks=1, short=0, long=0, conflict=1, observations=3)
    kept = tr.build_tracks_ref(img_ptr, edges, pair_ptr, pairs, conflicts=1, max_length=3)
    assert kept["feat_track"].tolist() == [0, 1, 0, 1, 1, 0] and kept["track_feat"].tolist() == [0, 2, 5, 1, 3, 4]
    both = tr.build_tracks_ref(img_ptr, edges, pair_ptr, pairs, min_length=4)
    assert both["feat_track"].tolist() == [-2, -3, -2, -3, -3, -2]
    assert both["counts"] == dict(components=2, tracks=0, short=1, long=0, conflict=1, observations=0)
    masked = tr.build_tracks_ref(img_ptr, edges, pair_ptr, pairs, pair_use=[1, 1, 0, 0])
    assert masked["feat_track"].tolist() == [0, 1, 0, 1, -1, -1]


GOOD = dict(img_ptr=[0, 2, 2, 5], edges=[(0, 2), (2, 0)], pair_ptr=[0, 2, 3], pairs=[(0, 1), (1, 2), (0, 1)])


@pytest.mark.parametrize("change", [
    dict(img_ptr=[1, 2, 2, 5]), dict(img_ptr=[0, 3, 2, 5]), dict(pair_ptr=[1, 2, 3]), dict(pair_ptr=[0, 3, 2, 3][:3]),
    dict(edges=[(0, 3), (2, 0)]), dict(edges=[(0, 2), (-1, 0)]), dict(edges=[(0, 2), (2, 2)]),
    dict(pairs=[(2, 1), (1, 2), (0, 1)]), dict(pairs=[(0, 1), (1, 3), (0, 1)]), dict(pairs=[(0, 1), (1, 2), (-1, 1)]),
    dict(edges=[(0, 1), (2, 0)]), dict(img_ptr=[0, 2, 2, 2 ** 31]), dict(min_length=0), dict(min_length=3, max_length=2),
    dict(max_length=-1), dict(conflicts=2), dict(pair_use=[1, 0]), dict(pair_ptr=[0, 2, 4]), dict(edges=[(0, 2)]),
    dict(pairs=[(0.5, 1), (1, 2), (0, 1)]),
], ids=lambda c: ",".join(f"{k}={v}" for k, v in c.items()).replace(" ", ""))
def test_check_track_inputs_refuses(change):
    import sfmba
    args = dict(GOOD)
    args.update(change)
    with pytest.raises(ValueError):
        sfmba.check_track_inputs(**args)


def test_check_track_inputs_accepts_the_valid_edge_cases():
    import sfmba
    img_ptr, edges, pair_ptr, pairs, use, opt = sfmba.check_track_inputs(**GOOD)
    assert (img_ptr.dtype, edges.dtype, pair_ptr.dtype, pairs.dtype) == (np.int64, np.int32, np.int64, np.int32)
    assert use is None and opt == dict(min_length=2, max_length=0, conflicts=0, profile=0)
    assert sfmba.check_track_inputs([0, 4], [], [0], [])[3].shape == (0, 2)                      # zero edges
    assert sfmba.check_track_inputs([0, 2, 4], [(0, 1)], [0, 0], [])[3].shape == (0, 2)          # zero pairs
    assert sfmba.check_track_inputs(pair_use=[0, 0, 0], **GOOD)[4].tolist() == [0, 0, 0]
    assert sfmba.check_track_inputs(min_length=3, max_length=3, conflicts=1, **GOOD)[5]["max_length"] == 3


def test_tracks_problem_on_five_features():
    import sfmba
    # image 0: two features, image 1: two, image 2: one; tracks {0, 2, 4} and {1, 3}
    img_ptr = np.array([0, 2, 4, 5], dtype=np.int64)
    ref = tr.build_tracks_ref(img_ptr, [(0, 1), (2, 1)], [0, 2, 3], [(0, 0), (1, 1), (0, 0)])
    t = sfmba.Tracks(img_ptr, ref["feat_track"], ref["track_ptr"], ref["track_feat"], ref["track_image"],
                     [ref["counts"][k] for k in tr.COUNTS], 0.0)
    pts = [np.array([[10., 11.], [20., 21.]]), np.array([[30., 31.], [40., 41.]]), np.array([[50., 51.]])]
    n_points, cam, pt, uv = t.problem(pts)
    assert n_points == 2 and t.n_tracks == 2 and t.counts["observations"] == 5
    assert cam.tolist() == [0, 1, 2, 0, 1] and pt.tolist() == [0, 0, 0, 1, 1]
    assert uv.tolist() == [[10., 11.], [30., 31.], [50., 51.], [20., 21.], [40., 41.]]
    assert t.track_row.tolist() == [0, 0, 0, 1, 1]
    assert t.track_of(1, 1) == 1 and t.track_of(2, 0) == 0 and t.track_of([0, 1], [1, 0]).tolist() == [1, 0]
    assert (t.UNMATCHED, t.SHORT, t.CONFLICT) == (-1, -2, -3)
    with pytest.raises(ValueError):
        t.track_of(2, 1)
    with pytest.raises(ValueError):
        t.problem(pts[:2])


def test_build_tracks_refuses_before_touching_the_device():
    import sfmba
    with pytest.raises(ValueError):
        sfmba.build_tracks([(0, 0, [(0, 0)])], [3, 3], device=10 ** 6)      # u == v; no such device is ever opened
    with pytest.raises(ValueError):
        sfmba.build_tracks([(0, 1, [(0, 3)], None, None)], [3, 3], device=10 ** 6)


def test_constants_come_from_the_source():
    assert tr.track_constant("kTrackScanItems") == tr.track_constant("kTrackBlock") * tr.track_constant("kTrackScanPerThread")
    assert tr.track_constant("kTrackLong") >= 2


def test_input_checks_under_sanitizers():
    subprocess.run(["make", "-C", PKG, "track-check"], check=True, capture_output=True, timeout=600)
    run = subprocess.run([os.path.join(PKG, "build", "track_inputs_check_asan")], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "track_inputs_check: ok" in run.stdout
