"""CPU-side checks of descriptor matching: the numpy restatement (tests/match_ref.py) against cases worked by hand, the
wrappers' argument validation (every malformed input raises ValueError before any device call), the compaction of
`DescriptorMatches.pairs`, the objects of `knn_match`, and the share of contested queries in every form-B fixture of the
GPU test."""
import numpy as np
import pytest

import match_ref as mr


def test_reference_on_hand_computed_cases():
    q = np.array([[0, 0], [3, 4], [10, 10]], dtype=np.uint8)
    t = np.array([[0, 1], [3, 4], [0, 2], [1, 0]], dtype=np.uint8)
    r = mr.match_edge(q, t)
    # query 0: d^2 = 1, 25, 4, 1 -> rows 0 and 3 tie at 1, the lower index first; 1 < 0.25 x 1 is false
    # query 1: d^2 = 18, 0, 13, 20 -> 0 < 0.25 x 13;  query 2: d^2 = 181, 85, 164, 181 -> 85 < 41 is false
    assert r["idx"].tolist() == [[0, 3], [1, 2], [1, 2]]
    assert r["dist_sq"].tolist() == [[1.0, 1.0], [0.0, 13.0], [85.0, 164.0]]
    assert r["good"].tolist() == [False, True, False] and r["status"] == mr.OK
    assert mr.good_pairs(q, t).tolist() == [[1, 1]]
    # the boundary is strict: (1, 4) fails, (1, 5) passes
    assert not mr.match_edge(np.zeros((1, 2), np.uint8), np.array([[1, 0], [2, 0]], np.uint8))["good"][0]
    assert mr.match_edge(np.zeros((1, 2), np.uint8), np.array([[1, 0], [2, 1]], np.uint8))["good"][0]
    # float input goes through fp64 differences and gives the same
    rf = mr.match_edge(q.astype(np.float32), t.astype(np.float32))
    assert rf["idx"].tolist() == r["idx"].tolist() and rf["dist_sq"].tolist() == r["dist_sq"].tolist()


def test_reference_statuses_and_non_finite_rows():
    q = np.zeros((2, 3), dtype=np.float32)
    for t in (np.zeros((1, 3), np.float32), np.zeros((0, 3), np.float32)):
        r = mr.match_edge(q, t)
        assert r["status"] == mr.FEW and (r["idx"] == -1).all() and not r["good"].any() and np.isinf(r["dist_sq"]).all()
    assert mr.match_edge(np.zeros((0, 3), np.float32), np.ones((5, 3), np.float32))["status"] == mr.FEW
    t = np.array([[np.nan, 0, 0], [1, 0, 0], [np.inf, 0, 0]], dtype=np.float32)
    r = mr.match_edge(q, t)
    assert r["status"] == mr.OK and r["idx"].tolist() == [[1, -1], [1, -1]] and not r["good"].any()
    assert r["dist_sq"][:, 0].tolist() == [1.0, 1.0] and np.isinf(r["dist_sq"][:, 1]).all()
    b = mr.match_batch([q, t, t[:1]], [(0, 1), (0, 2), (1, 1)])
    assert b["query_ptr"].tolist() == [0, 2, 4, 7] and b["edge_status"].tolist() == [0, 1, 0] and b["n_ok"] == 2
    assert b["idx"][4:].tolist() == [[-1, -1], [1, -1], [-1, -1]]       # u == v: only the finite row finds itself


def test_wrappers_validate_before_any_device_call():
    import sfmba
    d8 = [np.zeros((4, 8), np.uint8), np.ones((3, 8), np.uint8)]
    bad_sets = [
        np.zeros((4, 8), np.uint8),                              # one array, not a list of arrays
        [np.zeros(8, np.uint8)],                                 # not 2-D
        [np.zeros((4, 8), np.uint8), np.zeros((4, 9), np.uint8)],          # lengths differ
        [np.zeros((4, 513), np.float32)],                        # too long
        [np.zeros((4, 0), np.float32)],                          # too short
        [np.array([["a", "b"]])],                                # not numbers
        [np.zeros((2, 4), np.complex64)],
    ]
    for descs in bad_sets:
        with pytest.raises(ValueError):
            sfmba.match_descriptors(descs)
    for edges in ([(0, 2)], [(-1, 0)], [(0, 1, 1)], [(0.0, 1.0)], np.zeros((2, 2, 2), int)):
        with pytest.raises(ValueError):
            sfmba.match_descriptors(d8, edges)
    for kw in (dict(ratio=0.0), dict(ratio=-0.5), dict(ratio=float("nan")), dict(form=3)):
        with pytest.raises(ValueError):
            sfmba.match_descriptors(d8, **kw)
    for k in (1, 3):
        with pytest.raises(ValueError):
            sfmba.knn_match(d8[0], d8[1], k=k)
    with pytest.raises(ValueError):
        sfmba.knn_match(d8[0], np.zeros((3, 9), np.uint8))
    K = np.eye(3)
    pts = [np.zeros((4, 2)), np.zeros((3, 2))]
    for args in ((d8, pts[:1], K), (d8, [pts[0], np.zeros((4, 2))], K), (d8, pts, np.eye(4)), (bad_sets[2], pts, K)):
        with pytest.raises(ValueError):
            sfmba.match_features(*args)
    with pytest.raises(ValueError):
        sfmba.match_features(d8, pts, K, ratio=0.0)


def test_checked_descriptor_sets():
    from sfmba.backend import check_descriptors, check_match_edges
    desc, ptr = check_descriptors([np.zeros((4, 8), np.uint8), np.ones((0, 8), np.uint8), np.ones((3, 8), np.uint8)])
    assert desc.dtype == np.uint8 and desc.shape == (7, 8) and ptr.tolist() == [0, 4, 4, 7] and desc.flags.c_contiguous
    desc, ptr = check_descriptors([np.zeros((4, 8), np.uint8), np.ones((3, 8), np.float64)])
    assert desc.dtype == np.float32 and ptr.tolist() == [0, 4, 7]
    assert check_match_edges(None, 3).tolist() == [[1, 0], [2, 0], [2, 1]]           # the reference's order of u > v
    assert check_match_edges([], 3).shape == (0, 2) and check_match_edges((2, 1), 3).tolist() == [[2, 1]]
    assert check_match_edges([(0, 0)], 1).dtype == np.int32


def test_pairs_compaction():
    import sfmba
    idx = np.array([[4, 1], [0, 2], [7, 3], [-1, -1], [5, 6], [2, 0]], dtype=np.int32)
    good = np.array([1, 0, 1, 0, 1, 1], dtype=bool)
    m = sfmba.DescriptorMatches(np.array([[1, 0], [2, 0], [2, 1]], np.int32), np.array([0, 3, 4, 6]), idx, np.zeros((6, 2)),
                                good, np.array([2, 0, 2], np.int32), np.array([0, 1, 0], np.int32), 2, 0.0)
    assert m.pairs(0).tolist() == [[0, 4], [2, 7]]
    assert m.pairs(1).shape == (0, 2) and m.pairs(1).dtype == int
    assert m.pairs(2).tolist() == [[0, 5], [1, 2]]               # query indices count from the edge's first row


def test_knn_match_objects():
    from sfmba.extras import DMatch, dmatch_lists
    idx = np.array([[3, 1], [2, -1], [-1, -1]], dtype=np.int32)
    dist = np.array([[4.0, 10.0], [2.0, np.inf], [np.inf, np.inf]])
    out = dmatch_lists(idx, dist)
    assert [len(p) for p in out] == [2, 1, 0]
    m, n = out[0]
    assert isinstance(m, DMatch) and (m.queryIdx, m.trainIdx, m.distance) == (0, 3, 2.0)
    assert (n.queryIdx, n.trainIdx) == (0, 1) and n.distance == float(np.float32(np.sqrt(10.0)))
    assert out[1][0].queryIdx == 1 and out[1][0].trainIdx == 2
    good = [(a.queryIdx, a.trainIdx) for a, b in out[:1] if a.distance < 0.7 * b.distance]      # the reference's loop
    assert good == [(0, 3)]


@pytest.mark.parametrize("shape", mr.FORM_B_SHAPES)
def test_contested_share_of_the_form_b_fixtures(shape):
    q, t = mr.form_b_fixture(*shape)
    assert q.dtype == t.dtype == np.float32 and q.shape == (shape[1], shape[0]) and t.shape == (shape[2], shape[0])
    share = mr.contested(q, t).mean()
    print(f"{shape}: {share:.4f} contested")
    assert share <= mr.CONTESTED_CAP
    good = mr.match_edge(q, t)["good"].mean()
    assert 0.3 < good < 0.7
