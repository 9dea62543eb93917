"""CPU-side checks of the two-view feature: the numpy restatement (tests/two_view_ref.py) against the reference's recorded
estimate_fundamental_matrix / estimate_fundamental_matrix_ransac / recover_pose output, the sample rule, the header /
binding / built library, and the argument checks of the Python layer.  No GPU compute is called here."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import two_view_ref as tv

LIB = os.path.join(ROOT, "sfm-python_amd", "sfmba", "libsfmba.so")
BOUNDS = json.load(open(os.path.join(GOLDEN, "two_view_bounds.json")))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__ as ge
        ge.build()
    return ctypes.CDLL(LIB)


@pytest.fixture(scope="module")
def cases():
    return tv.load_cases(GOLDEN)


def test_fixture_is_data_of_the_expected_shape(cases):
    ransac, pose, K = cases
    want = [[n, z, 0.1] for n in (8, 9, 64, 257) for z in (0.0, 0.05)] + [[1000, 0.3, 1.0]]
    assert [[c["n"], c["noise"], c["threshold"]] for c in ransac] == want == BOUNDS["ransac_cases"]
    assert [[c["n"], c["noise"]] for c in pose] == [[n, z] for n in (8, 64, 257) for z in (0.0, 0.3)] == BOUNDS["pose_cases"]
    H = BOUNDS["hypotheses"]
    assert H == 200 and BOUNDS["factor"] == 100.0 and K.shape == (3, 3)
    for c in ransac:
        assert c["samples"].shape == (H, 8) and c["samples"].dtype == np.int32 and c["hyp_masks"].shape == (H, c["n"])
        assert np.array_equal(c["hyp_masks"].sum(axis=1), c["hyp_inliers"])
        assert c["best"] == int(np.argmax(c["hyp_inliers"])) and np.array_equal(c["mask"], c["hyp_masks"][c["best"]])
    for key in ("F_hyp", "F_refit", "R_angle", "t_dist"):
        assert BOUNDS[key]["bound"] == BOUNDS["factor"] * BOUNDS[key]["measured_max"]
    # the conditions under which masks and counts must be exactly equal
    assert BOUNDS["flipped_masks"] == 0 and BOUNDS["nearest_distance_over_threshold"] > 1e-6
    assert BOUNDS["scored_pairs"] == H * sum(c["n"] for c in ransac)


def test_restatement_matches_the_reference_ransac(cases):
    """Per hypothesis: F within the bound, the mask equal; per case: counts, best, mask equal, the refit within its bound."""
    worst = dict(F_hyp=0.0, F_refit=0.0)
    for c in cases[0]:
        thr = c["threshold"]
        out = tv.ransac_edge(c["pts1"], c["pts2"], c["samples"], threshold=thr, refit=True, margin=1e-6 * thr)
        assert not out["near"].any()
        assert np.array_equal(out["hyp"], c["hyp_inliers"]) and out["best"] == c["best"] and out["inliers"] == c["inliers"]
        assert np.array_equal(out["mask"], c["mask"]) and out["success"] == c["success"]
        assert out["status"] == (tv.OK if c["inliers"] >= 8 else tv.DEGENERATE)
        for h in range(len(c["samples"])):
            assert np.array_equal(tv.inliers(out["hyp_F"][h], c["pts1"], c["pts2"], thr), c["hyp_masks"][h])
            d = float(np.abs(tv.unit_F(out["hyp_F"][h]) - tv.unit_F(c["hyp_F"][h])).max())
            assert d <= BOUNDS["F_hyp"]["bound"], (c["n"], c["noise"], h, d)
            worst["F_hyp"] = max(worst["F_hyp"], d)
        if out["status"] == tv.OK:
            assert np.abs(out["F"] - c["F"]).max() <= BOUNDS["F_hyp"]["bound"]
            d = float(np.abs(out["F_refit"] - c["F_refit"]).max())
            assert d <= BOUNDS["F_refit"]["bound"], (c["n"], c["noise"], d)
            worst["F_refit"] = max(worst["F_refit"], d)
    for key, val in worst.items():
        print(f"{key}: {val:.3e} (recorded {BOUNDS[key]['measured_max']:.3e}, bound {BOUNDS[key]['bound']:.3e})")
        assert val <= 10 * BOUNDS[key]["measured_max"]


def test_restatement_matches_the_reference_pose(cases):
    _, pose, K = cases
    for c in pose:
        out = tv.recover_pose_edge(c["E"], c["pts1"], c["pts2"], K)
        assert out["status"] == tv.OK and np.array_equal(out["mask"], c["mask"]) and out["front"] == c["mask"].sum()
        assert np.all(np.delete(out["front_all"], int(np.argmax(out["front_all"]))) < out["front"])
        assert tv.rotation_angle(c["R"], out["R"]) <= BOUNDS["R_angle"]["bound"], (c["n"], c["noise"])
        assert np.linalg.norm(c["t"] - out["t"]) <= BOUNDS["t_dist"]["bound"], (c["n"], c["noise"])
        assert abs(np.linalg.norm(out["t"]) - 1.0) <= 1e-15 and abs(np.linalg.det(out["R"]) - 1.0) <= 1e-14
        # the four candidates: both rotations proper, the translations opposite
        cands, _ = tv.decompose(c["E"])
        assert all(abs(np.linalg.det(R) - 1.0) <= 1e-14 for R, _ in cands)
        assert np.array_equal(cands[0][1], -cands[1][1]) and np.array_equal(cands[0][0], cands[1][0])
        # exact pixels: the linear points reproject onto them (pixels ~1e3 to 1e-13, through an E of condition ~1e3)
        if c["noise"] == 0.0:
            assert out["sum_err"] <= 1e-6 * c["n"], (c["n"], out["sum_err"])


def test_sample_rule():
    assert hex(tv.mix(1)) == "0x5692161d100b05e5"
    assert tv.draw_sample(12345, 3, 17, 100) == [60, 53, 54, 45, 8, 82, 79, 32]
    assert tv.draw_sample(2 ** 64 - 1, 256, 999, 5000) == [2839, 2449, 89, 1984, 3064, 4256, 75, 4439]
    assert tv.draw_sample(0, 0, 0, 8) == [7, 1, 2, 6, 5, 0, 4, 3]
    seen = set()
    for n in (8, 9, 10, 64, 1000):
        for e in (0, 1, 4949):
            for h in range(40):
                s = tv.draw_sample(99, e, h, n)
                assert len(set(s)) == 8 and min(s) >= 0 and max(s) < n
                if n == 8:
                    assert sorted(s) == list(range(8))
                seen.add((n, tuple(s)))
    assert len(seen) > 0.9 * 5 * 3 * 40 - 120                    # (n = 8 has only permutations; the others hardly repeat)
    # e and h enter separately: (e, h) and (h, e) differ
    assert tv.draw_sample(5, 1, 2, 50) != tv.draw_sample(5, 2, 1, 50)
    s = tv.draw_samples(7, 0, 3, 20)
    assert s.shape == (3, 8) and s.dtype == np.int32


def test_header_binding_and_library_agree(lib):
    import sfmba
    from sfmba import _capi
    header = open(os.path.join(ROOT, "include", "sfmba.h")).read()
    assert re.search(r"\bint\s+sfmba_fundamental_ransac\(sfmba_handle\* h, int64_t n_edges, const int64_t\* edge_ptr", header)
    assert re.search(r"\bint\s+sfmba_recover_pose\(sfmba_handle\* h, int64_t n_edges, const int64_t\* edge_ptr", header)
    assert "NOT OpenCV's" in header
    for name in ("sfmba_default_ransac_options", "sfmba_fundamental_ransac", "sfmba_default_pose_options", "sfmba_recover_pose"):
        assert name in _capi.SYMBOLS and hasattr(lib, name), name
    for name in ("FundamentalEstimate", "RelativePose", "find_fundamental_mat", "recover_pose", "select_initial_pair"):
        assert name in sfmba.__all__ and hasattr(sfmba, name), name
    ctype = {"int32_t": ctypes.c_int32, "double": ctypes.c_double, "uint64_t": ctypes.c_uint64}
    for T, cname, size in ((_capi.RansacOptions, "sfmba_ransac_options", 40), (_capi.PoseOptions, "sfmba_pose_options", 16)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), header, re.S).group(1)
        fields = re.findall(r"^\s*(int32_t|double|uint64_t)\s+(\w+);", body, re.M)
        assert [(name, ctype[t]) for t, name in fields] == list(T._fields_)
        assert ctypes.sizeof(T) == size

        class Guarded(ctypes.Structure):
            _fields_ = [("o", T), ("guard", ctypes.c_uint64)]
        g = Guarded()
        g.guard = 0xA5A5A5A5A5A5A5A5
        fn = getattr(lib, "sfmba_default_" + cname[len("sfmba_"):])
        fn.argtypes, fn.restype = [ctypes.POINTER(T)], None
        fn(ctypes.cast(ctypes.byref(g), ctypes.POINTER(T)))
        assert g.guard == 0xA5A5A5A5A5A5A5A5
        if T is _capi.RansacOptions:
            assert (g.o.threshold, g.o.confidence, g.o.seed, g.o.max_iters, g.o.refit, g.o.profile) == (1.0, 0.99, 0, 1000, 0, 0)
        else:
            assert (g.o.min_depth, g.o.profile) == (0.0, 0)
    from kernel_source import kernel_constant
    assert kernel_constant("kTwoViewLdsPairs") * 32 + 8192 <= 160 * 1024     # the staged pairs beside the kernel's static LDS


def test_python_layer_rejects_bad_arguments():
    """Checked before any handle is made, so no GPU is needed."""
    import sfmba
    from sfmba.backend import _edge_batch
    p = np.zeros((10, 2))
    with pytest.raises(ValueError, match=r"\(M, 2\)"):
        _edge_batch(np.zeros((10, 3)), p, None, None)
    with pytest.raises(ValueError, match=r"\(M, 2\)"):
        _edge_batch(p, p[:9], None, None)
    with pytest.raises(ValueError, match="edge_ptr"):
        _edge_batch(p, p, [0, 4, 9], None)
    with pytest.raises(ValueError, match="edge_ptr"):
        _edge_batch(p, p, [0, 6, 4, 10], None)
    with pytest.raises(ValueError, match="pair_use"):
        _edge_batch(p, p, None, np.ones(9))
    a, b, ptr, use = _edge_batch(p, p, None, np.arange(10))
    assert ptr.tolist() == [0, 10] and ptr.dtype == np.int64 and use.tolist() == [0] + [1] * 9 and use.dtype == np.uint8
    assert _edge_batch(p, p, [0, 3, 3, 10], None)[2].tolist() == [0, 3, 3, 10]
    with pytest.raises(ValueError, match="FM_RANSAC"):
        sfmba.find_fundamental_mat(p, p, method=4)
    with pytest.raises(ValueError):
        sfmba.find_fundamental_mat(p, p[:5])
    with pytest.raises(ValueError):
        sfmba.recover_pose(np.eye(3), p, p[:, :1], np.eye(3))
    with pytest.raises(ValueError):
        sfmba.recover_pose(np.zeros((2, 3, 3)), p, p, np.eye(3))
    with pytest.raises(ValueError, match="empty"):
        sfmba.select_initial_pair([], np.eye(3))
    with pytest.raises(ValueError):
        sfmba.select_initial_pair([(p, p[:4])], np.eye(3))
    assert sfmba.FM_RANSAC == 8
