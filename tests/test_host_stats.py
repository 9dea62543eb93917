"""CPU-side checks of the reprojection-statistics feature: `prune_problem` (pure numpy) on hand-built masks, and the new
entry points and struct layouts of the built library.  No GPU compute is called here."""
import ctypes
import os

import numpy as np
import pytest

from conftest import ROOT

LIB = os.path.join(ROOT, "sfm-python_amd", "sfmba", "libsfmba.so")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__ as ge
        ge.build()
    return ctypes.CDLL(LIB)


def _problem():
    """3 cameras, 5 points, 9 observations in no particular order; every value distinct so rows can be told apart."""
    C, P = 3, 5
    ci = np.array([0, 1, 2, 0, 1, 2, 0, 1, 2], dtype=np.int64)
    pi = np.array([4, 0, 1, 1, 3, 0, 2, 2, 4], dtype=np.int64)
    uv = np.arange(18, dtype=np.int64).reshape(9, 2) * 10
    K = np.diag([100.0, 100.0, 1.0])
    x = np.arange(6 * C + 3 * P, dtype=np.float64) + 0.5
    return x, (C, P, ci, pi, uv, K)


def test_prune_renumbers_points_and_keeps_order():
    from sfmba import prune_problem
    x, args = _problem()
    C, P, ci, pi, uv, K = args
    obs_keep = np.array([1, 1, 0, 1, 1, 1, 1, 1, 1], dtype=bool)
    pt_keep = np.array([1, 1, 0, 1, 1], dtype=bool)                 # point 2 goes, and with it observations 6, 7
    x2, args2, oi, pti = prune_problem(x, args, obs_keep, pt_keep)
    assert list(oi) == [0, 1, 3, 4, 5, 8]                           # ascending: the original order
    assert list(pti) == [0, 1, 3, 4]
    C2, P2, ci2, pi2, uv2, K2 = args2
    assert (C2, P2) == (3, 4)                                       # all cameras stay
    # the index maps reproduce the kept rows of the original arrays
    assert np.array_equal(ci2, ci[oi]) and np.array_equal(uv2, uv[oi])
    assert np.array_equal(pti[pi2], pi[oi])                         # dense new ids point at the same old points
    assert list(pi2) == [3, 0, 1, 2, 0, 3]
    assert np.array_equal(x2[:18], x[:18])
    assert np.array_equal(x2[18:].reshape(-1, 3), x[18:].reshape(-1, 3)[pti])
    assert K2 is K or np.array_equal(K2, K)
    assert x2.shape[0] == 6 * C2 + 3 * P2 and uv2.dtype == uv.dtype


def test_prune_all_kept_returns_equal_arrays():
    from sfmba import prune_problem
    x, args = _problem()
    x2, args2, oi, pti = prune_problem(x, args, np.ones(9, dtype=np.uint8), np.ones(5, dtype=np.uint8))
    assert np.array_equal(x2, x)
    assert args2[0] == args[0] and args2[1] == args[1]
    for a, b in zip(args2[2:], args[2:]):
        assert np.array_equal(a, b)
    assert np.array_equal(oi, np.arange(9)) and np.array_equal(pti, np.arange(5))


def test_prune_dropped_point_takes_its_kept_observations():
    from sfmba import prune_problem
    x, args = _problem()
    pt_keep = np.array([0, 1, 1, 1, 1], dtype=bool)                 # point 0: observations 1 and 5, both marked kept
    x2, args2, oi, pti = prune_problem(x, args, np.ones(9, dtype=bool), pt_keep)
    assert list(oi) == [0, 2, 3, 4, 6, 7, 8]
    assert list(pti) == [1, 2, 3, 4]
    assert args2[3].min() == 0 and args2[3].max() == 3
    assert np.array_equal(pti[args2[3]], args[3][oi])


def test_prune_can_leave_a_camera_without_observations():
    from sfmba import prune_problem
    x, args = _problem()
    obs_keep = args[2] != 2                                          # every observation of camera 2 goes
    x2, args2, oi, pti = prune_problem(x, args, obs_keep, np.ones(5, dtype=bool))
    assert args2[0] == 3 and 2 not in args2[2]
    assert np.array_equal(x2, x)                                     # no point was dropped: same parameters


@pytest.mark.parametrize("n_obs_mask, n_pt_mask", [(8, 5), (10, 5), (9, 4), (9, 6), (0, 5)])
def test_prune_wrong_mask_lengths_raise(n_obs_mask, n_pt_mask):
    from sfmba import prune_problem
    x, args = _problem()
    with pytest.raises(ValueError):
        prune_problem(x, args, np.ones(n_obs_mask, dtype=bool), np.ones(n_pt_mask, dtype=bool))


def test_prune_wrong_x_length_raises():
    from sfmba import prune_problem
    x, args = _problem()
    with pytest.raises(ValueError):
        prune_problem(x[:-1], args, np.ones(9, dtype=bool), np.ones(5, dtype=bool))


def test_library_exports_the_statistics_entry_points(lib):
    from sfmba import _capi
    for name in ("sfmba_default_filter_options", "sfmba_reprojection_stats"):
        assert name in _capi.SYMBOLS
        assert hasattr(lib, name), name
    header = open(os.path.join(ROOT, "include", "sfmba.h")).read()
    assert "typedef struct sfmba_filter_options" in header and "typedef struct sfmba_stats_summary" in header


def test_statistics_struct_layouts_and_defaults(lib):
    from sfmba import _capi
    assert ctypes.sizeof(_capi.FilterOptions) == 32                  # 3 doubles, 2 int32
    assert ctypes.sizeof(_capi.StatsSummary) == 56                   # 4 int64, 3 doubles
    assert _capi.FilterOptions.min_views.offset == 24 and _capi.StatsSummary.sum_err.offset == 32
    lib.sfmba_default_filter_options.argtypes = [ctypes.POINTER(_capi.FilterOptions)]
    lib.sfmba_default_filter_options.restype = None
    # the library writes exactly sizeof(struct) bytes: a guard word behind the struct stays as it was
    class Guarded(ctypes.Structure):
        _fields_ = [("o", _capi.FilterOptions), ("guard", ctypes.c_uint64)]
    g = Guarded()
    g.guard = 0xA5A5A5A5A5A5A5A5
    lib.sfmba_default_filter_options(ctypes.cast(ctypes.byref(g), ctypes.POINTER(_capi.FilterOptions)))
    assert g.guard == 0xA5A5A5A5A5A5A5A5
    assert g.o.max_error_px == np.inf and g.o.min_depth == -np.inf
    assert g.o.min_angle_deg == 0.0 and g.o.min_views == 0 and g.o.reserved == 0
