"""CPU-side checks of the homography feature: header / binding / built library, the four-draw sample rule, the argument
checks of the Python layer, and the numpy restatement (tests/homography_ref.py) on exact planar pairs.  No GPU compute is
called here."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

import homography_ref as hr
import two_view_ref as tv

LIB = os.path.join(ROOT, "sfm-python_amd", "sfmba", "libsfmba.so")
K = np.array([[2905.88, 0.0, 1416.0], [0.0, 2905.88, 1064.0], [0.0, 0.0, 1.0]])


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__ as ge
        ge.build()
    return ctypes.CDLL(LIB)


def test_header_binding_and_library_agree(lib):
    import sfmba
    from sfmba import _capi
    header = open(os.path.join(ROOT, "include", "sfmba.h")).read()
    m = re.search(r"\bint\s+sfmba_homography_ransac\(sfmba_handle\* h, int64_t n_edges, const int64_t\* edge_ptr, const double\* pts1, "
                  r"const double\* pts2,(.*?)\);", header, re.S)
    assert m
    names = re.findall(r"(\w+)\s*(?:/\*.*?\*/)?\s*(?:,|$)", m.group(1), re.S)
    assert names == ["pair_use", "samples", "opt", "Hm", "H_refit", "inlier_mask", "refit_mask", "edge_inliers", "edge_refit_inliers",
                     "edge_best", "edge_success", "edge_status", "hyp_inliers", "n_ok", "kernel_us"]
    assert "const sfmba_ransac_options* opt" in m.group(1) and "STRICTLY below threshold^2" in header
    assert "sfmba_homography_ransac" in _capi.SYMBOLS and hasattr(lib, "sfmba_homography_ransac")
    assert len(_capi.load().sfmba_homography_ransac.argtypes) == 5 + len(names)
    for name in ("HomographyEstimate", "find_homography", "RANSAC"):
        assert name in sfmba.__all__ and hasattr(sfmba, name), name
    assert sfmba.RANSAC == 8
    assert (sfmba.HomographyEstimate.OK, sfmba.HomographyEstimate.FEW_PAIRS, sfmba.HomographyEstimate.DEGENERATE) == (0, 1, 2)
    assert hasattr(sfmba.Backend, "homography_ransac")


def test_sample_rule_of_four_draws():
    # the four draws are the first four of the F call's eight: the same key, the same update
    for seed, e, h, n in ((12345, 3, 17, 100), (2 ** 64 - 1, 256, 999, 5000), (0, 0, 0, 8)):
        assert hr.draw_sample4(seed, e, h, n) == tv.draw_sample(seed, e, h, n)[:4]
    seen = set()
    for n in (4, 5, 6, 64, 1000):
        for e in (0, 1, 4949):
            for h in range(40):
                s = hr.draw_sample4(99, e, h, n)
                assert len(set(s)) == 4 and min(s) >= 0 and max(s) < n
                if n == 4:
                    assert sorted(s) == [0, 1, 2, 3]
                seen.add((n, tuple(s)))
    assert len({s for n, s in seen if n == 4}) > 12              # (of the 24 permutations)
    assert len({s for n, s in seen if n >= 64}) > 0.9 * 2 * 3 * 40
    # e and h enter separately: (e, h) and (h, e) differ
    assert hr.draw_sample4(5, 1, 2, 50) != hr.draw_sample4(5, 2, 1, 50)
    s = hr.draw_samples4(7, 0, 3, 20)
    assert s.shape == (3, 4) and s.dtype == np.int32


def test_python_layer_rejects_bad_arguments():
    """Checked before any handle is made, so no GPU is needed."""
    import sfmba
    from sfmba import _capi
    from sfmba.backend import _ransac_prologue

    def _homography_samples(samples, n_edges):                   # as Backend.homography_ransac hands them over
        return _ransac_prologue(_capi.RansacOptions(max_iters=1000), {}, samples, n_edges, 4, "n_edges", "edge", "RANSAC",
                                strict=True)
    assert _homography_samples(None, 3) is None
    good = _homography_samples(np.zeros((2, 5, 4), dtype=np.int64), 2)
    assert good.dtype == np.int32 and good.shape == (2, 5, 4) and good.flags.c_contiguous
    for bad in (np.zeros((2, 5, 8), dtype=np.int32), np.zeros((5, 4), dtype=np.int32), np.zeros((3, 5, 4), dtype=np.int32),
                np.zeros((2, 0, 4), dtype=np.int32), np.zeros((2, 5, 4), dtype=np.float64), np.zeros((2, 5, 4, 1), dtype=np.int32)):
        with pytest.raises(ValueError, match=r"\(n_edges, H, 4\)"):
            _homography_samples(bad, 2)
    p = np.zeros((10, 2))
    with pytest.raises(ValueError, match="RANSAC"):
        sfmba.find_homography(p, p, method=0)
    with pytest.raises(ValueError, match="RANSAC"):
        sfmba.find_homography(p, p, method=4)
    with pytest.raises(ValueError):
        sfmba.find_homography(p, p[:5])
    with pytest.raises(ValueError):
        sfmba.find_homography(p[:, :1], p[:, :1])
    with pytest.raises(ValueError, match="max_homography_ratio"):
        sfmba.select_initial_pair([(p, p)], np.eye(3), max_homography_ratio=-1.0)
    with pytest.raises(ValueError, match="max_homography_ratio"):
        sfmba.select_initial_pair([(p, p)], np.eye(3), max_homography_ratio=np.nan)
    with pytest.raises(ValueError, match="empty"):
        sfmba.select_initial_pair([], np.eye(3), max_homography_ratio=0.8)


def test_restatement_recovers_the_generating_homography():
    rng = np.random.default_rng(31)
    for n, baseline in ((4, 1.0), (5, 1.0), (9, 0.0), (64, 1.0), (300, 0.0)):
        p1, p2, Hm, _, _, _ = hr.planar_pairs(rng, n, K, baseline=baseline)
        d = np.abs(hr.unit_H(hr.estimate_H(p1, p2)) - hr.unit_H(Hm)).max()
        assert d <= 1e-9, (n, baseline, d)
        assert np.sqrt(hr.distances_sq(Hm, p1, p2)).max() <= 1e-9
    # ... and through the RANSAC of the restatement, outliers and all
    p1, p2, Hm, _, _, bad = hr.planar_pairs(rng, 60, K, outliers=0.25)
    out = hr.ransac_edge(p1, p2, hr.draw_samples4(1, 0, 50, 60), threshold=1.0, refit=True)
    assert out["status"] == hr.OK and np.array_equal(out["mask"], ~bad) and np.array_equal(out["refit_mask"], ~bad)
    assert out["inliers"] == out["refit_inliers"] == 45 and out["best"] == int(np.argmax(out["hyp"]))
    assert np.abs(out["H_refit"] - hr.unit_H(Hm)).max() <= 1e-9 and np.abs(out["H"] - hr.unit_H(Hm)).max() <= 1e-9
    assert abs(np.linalg.norm(out["H"]) - 1.0) <= 4e-16 and out["H"].ravel()[np.argmax(np.abs(out["H"]))] > 0
    # the statuses that need no device
    assert hr.ransac_edge(p1[:3], p2[:3], np.zeros((2, 4), dtype=np.int32))["status"] == hr.FEW_PAIRS
    rep = hr.ransac_edge(p1, p2, np.zeros((2, 4), dtype=np.int32))
    assert rep["status"] == hr.DEGENERATE and rep["best"] == -1 and np.all(rep["hyp"] == -1) and not rep["H"].any()
