"""Host-side tests of the covariance call: the two routes of the CPU reference (tests/covariance_ref.py) against each other
and against the recorded bounds, the bounds file against a regeneration, the held-set rule, the device-free C++ part
(csrc/cov_inputs.hpp) as a stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer, and the exports.  No GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import covariance_ref as ref
from conftest import ROOT

PKG = os.path.join(ROOT, "sfm-python_amd")


@pytest.mark.parametrize("name", ["c3", "c11_dup", "grid21", "cond40"])
def test_routes_agree_within_the_recorded_spread(name):
    """The spread is a measurement of the routes themselves, so a regeneration reproduces it up to the order in which the
    BLAS of this machine sums (its thread count changes it): within ten times the recorded figure, a tenth of the factor
    the GPU is allowed."""
    rec, want = ref.case_bounds(name), ref.load_bounds()["cases"][name]
    for key in ("spread_cam", "spread_cam_cov", "spread_pt"):
        assert rec[key] <= 10.0 * want[key], (key, rec[key], want[key])
    assert ref.accept(name, rec) is None
    assert rec["gauge"] == want["gauge"] and rec["dof"] == want["dof"]
    for key in ("min_pivot_rel", "pt_min_pivot"):
        assert abs(rec[key] - want[key]) <= 1e-6 * want[key], key


def test_bounds_file_matches_a_regeneration_of_one_case():
    b = ref.load_bounds()
    assert b["factor"] == ref.FACTOR == 100.0 and b["rank_tol"] == ref.RANK_TOL and b["point_tol"] == ref.POINT_TOL
    assert sorted(b["cases"]) == sorted(ref.CASES)
    rec, want = ref.case_bounds("c3"), b["cases"]["c3"]
    assert sorted(rec) == sorted(want)
    assert rec["gauge"] == want["gauge"] == [0, 1, 0] and rec["dof"] == want["dof"]
    for key in ("spread_cam", "spread_cam_cov", "spread_pt"):          # same routes, same machine arithmetic: the same figure up to
        assert 0.1 * want[key] <= rec[key] <= 10.0 * want[key], key     # the BLAS's order of summation
    for key in ("min_pivot_rel", "pt_min_pivot", "eighth_eig_rel"):
        assert abs(rec[key] - want[key]) <= 1e-6 * want[key], key
    assert rec["null_eig_rel"] < ref.RANK_TOL


def test_reference_failures():
    c = ref.case("c3_undropped")
    out = ref.covariance(c["x"], c["args"])
    assert out["status"] == 2 and out["n_bad_points"] == 3 and list(np.nonzero(out["pt_status"] == 1)[0]) == [2, 4, 16]
    c = ref.case("c11_nogauge")
    out = ref.covariance(c["x"], c["args"], gauge=False)
    assert out["status"] == 1 and out["bad_param"] == 59 and (out["held"] == 0).all()


def test_held_mask_rule():
    x = np.zeros(6 * 4 + 3)
    x[3:6], x[9:12], x[15:18], x[21:24] = (0, 0, 0), (1, 0, 0), (0, -3, 1), (0, 3, -1)
    ci = np.array([0, 1, 2, 3])
    mask, g = ref.held_mask(x, 4, ci)
    assert g == (0, 2, 1) and mask.sum() == 7 and mask[6 * 2 + 4] == 1
    mask, g = ref.held_mask(x, 4, ci, fixed=(3,))
    assert g == (3, 2, 1) and mask[18:24].all()
    mask, g = ref.held_mask(x, 4, ci, fixed=(1, 3))
    assert g == (-1, -1, -1) and mask.sum() == 12
    mask, g = ref.held_mask(x, 4, ci, hold=(5,))
    assert g == (-1, -1, -1) and mask.sum() == 1
    mask, g = ref.held_mask(x, 4, np.array([0, 1, 3]))
    assert g == (0, 3, 1) and (mask[12:18] == 2).all()
    assert ref.held_mask(x, 4, ci, gauge=False)[0].sum() == 0


def test_block_error_is_scale_free():
    rng = np.random.default_rng(0)
    a = rng.normal(size=(5, 3, 3))
    a = a @ a.transpose(0, 2, 1)
    b = a * (1.0 + 1e-9)
    d = np.array([1e-6, 1.0, 1e6])
    s = d[:, None] * d[None, :]
    assert abs(ref.block_error(b, a) - ref.block_error(b * s, a * s)) < 1e-15
    z = np.zeros((2, 2))
    assert ref.block_error(z, z) == 0.0 and ref.block_error(np.array([[0.0, 1.0], [1.0, 0.0]]), z) == np.inf


def test_cov_inputs_under_sanitizers():
    subprocess.run(["make", "-C", PKG, "cov-check"], check=True, capture_output=True, timeout=600)
    run = subprocess.run([os.path.join(PKG, "build", "cov_inputs_check_asan")], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "cov_inputs_check: ok" in run.stdout


def test_library_exports_the_covariance_symbols():
    from sfmba import _capi
    assert {"sfmba_default_covariance_options", "sfmba_covariance"} <= set(_capi.SYMBOLS)
    lib = ctypes.CDLL(_capi.LIB_PATH)
    for s in ("sfmba_default_covariance_options", "sfmba_covariance"):
        assert hasattr(lib, s), s
    assert ctypes.sizeof(_capi.CovarianceOptions) == 40 and ctypes.sizeof(_capi.CovarianceInfo) == 88
    header = open(os.path.join(ROOT, "include", "sfmba.h")).read()
    assert "sfmba_covariance(" in header and "sfmba_covariance_info" in header
