"""CPU-side checks of the triangulation feature: the numpy restatement (tests/triangulate_ref.py) against the reference's
recorded two-view output and against numpy's own eigensolver, the option struct of the built library against `_capi`, and
the input checks of `sfmba.triangulate_points`.  No GPU compute is called here."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import triangulate_ref as tr

LIB = os.path.join(ROOT, "sfm-python_amd", "sfmba", "libsfmba.so")
EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__ as ge
        ge.build()
    return ctypes.CDLL(LIB)


@pytest.fixture(scope="module")
def cases():
    return np.load(os.path.join(GOLDEN, "triangulate_cases.npz"), allow_pickle=False)


def _two_view_problem(g):
    n = g["pts1"].shape[1]
    cams = np.concatenate([tr.cameras_from_projection(g["M1"], g["K"]), tr.cameras_from_projection(g["M2"], g["K"])])
    uv = np.stack([g["pts1"].T, g["pts2"].T], axis=1).reshape(2 * n, 2)
    args = (2, n, np.tile([0, 1], n), np.repeat(np.arange(n), 2), uv, g["K"])
    return np.concatenate([cams, np.zeros(3 * n)]), args


def test_fixture_is_data_of_the_expected_shape(cases):
    assert set(cases.files) == {"K", "M1", "M2", "pts1", "pts2", "X_ref"}
    n = cases["pts1"].shape[1]
    assert n >= 64 and cases["pts1"].shape == cases["pts2"].shape == (2, n)
    assert cases["M1"].shape == cases["M2"].shape == (3, 4) and cases["X_ref"].shape == (4, n)
    assert np.array_equal(cases["X_ref"][3], np.ones(n))


def test_restatement_matches_the_reference_on_the_fixture(cases):
    """The smallest eigenvector of A^T A by Jacobi rotations against the reference's SVD of A.  Bound per pair: an
    eigenvector computed with a backward error of a few eps |A^T A| is off by that over the gap to the next eigenvalue
    (Davis-Kahan); the constant 32 covers the 4x4 products and the camera round trip K^-1 M -> rotation vector -> M; the
    division by v[3] carries it to X as |(X, 1)|^2 times the eigenvector's error."""
    x, args = _two_view_problem(cases)
    out = tr.triangulate(x, args, max_iter=0, min_angle_deg=-np.inf, min_depth=-np.inf)
    assert np.all(out["status"] == tr.OK)
    X_ref = cases["X_ref"][:3].T
    M = tr.projection_matrices(x, 2, cases["K"])
    worst = 0.0
    for p in range(len(X_ref)):
        rows = tr.dlt_rows(M, args[4][2 * p:2 * p + 2])
        lam = np.linalg.eigvalsh(rows.T @ rows)
        bound = 32 * EPS * lam[3] / (lam[1] - lam[0]) * (1.0 + X_ref[p] @ X_ref[p])
        d = np.abs(out["linear"][p] - X_ref[p]).max()
        worst = max(worst, d)
        assert d <= bound, (p, d, bound)
    # ... and the recorded distance, which the GPU test's bound is 100 times of, is what this machine measures too
    rec = json.load(open(os.path.join(GOLDEN, "triangulate_bounds.json")))
    print(f"restatement vs reference: {worst:.3e} (recorded {rec['fixture']['measured_abs']:.3e})")
    assert rec["fixture"]["bound_abs"] == rec["factor"] * rec["fixture"]["measured_abs"] and rec["factor"] == 100.0
    assert worst <= 10 * rec["fixture"]["measured_abs"]


def test_jacobi_eigenvector_against_eigh():
    rng = np.random.default_rng(5)
    for k in range(50):
        rows = rng.normal(size=(2 * (2 + k % 5), 4)) * np.array([3000.0, 3000.0, 1500.0, 9000.0])
        A = rows.T @ rows
        w, V = np.linalg.eigh(A)
        v = tr.jacobi_smallest_eigenvector(A)
        assert abs(np.sqrt(v @ v) - 1.0) <= 16 * EPS
        sin = np.linalg.norm(v - V[:, 0] * (V[:, 0] @ v))               # the part of v outside eigh's eigenvector
        assert sin <= 32 * EPS * w[3] / (w[1] - w[0]), (k, sin)
    # diagonal input: no rotation at all, the unit vector of the smallest entry
    assert np.array_equal(tr.jacobi_smallest_eigenvector(np.diag([4.0, 1.0, 3.0, 2.0])), np.array([0.0, 1.0, 0.0, 0.0]))


def test_restatement_refinement_never_raises_the_cost():
    from sfmba.synthetic import make_problem
    pb = make_problem(4, 30, 150, seed=1)
    C, P, ci, pi, uv, K = pb.args
    lin = tr.triangulate(pb.x_true, pb.args, max_iter=0, min_angle_deg=0.0)
    ref = tr.triangulate(pb.x_true, pb.args, min_angle_deg=0.0)
    order, ptr = tr.stored_runs(pi, P)
    cams = pb.x_true[:6 * C].reshape(C, 6)
    both = np.flatnonzero((lin["status"] == tr.OK) & (ref["status"] == tr.OK))
    assert len(both) >= 20
    for p in both:
        idx = order[ptr[p]:ptr[p + 1]]
        assert tr.cost(ref["points"][p], cams, ci[idx], uv[idx], K) <= tr.cost(lin["points"][p], cams, ci[idx], uv[idx], K)
    assert np.all(ref["rms_err"][both] <= lin["rms_err"][both]) and ref["iters"].max() <= 10 and np.all(lin["iters"] == 0)


def test_library_exports_the_triangulation_entry_points(lib):
    from sfmba import _capi
    for name in ("sfmba_default_triangulate_options", "sfmba_triangulate"):
        assert name in _capi.SYMBOLS
        assert hasattr(lib, name), name


def test_option_struct_layout_and_defaults(lib):
    from sfmba import _capi
    T = _capi.TriangulateOptions
    # the header's fields, in order, are the binding's
    header = open(os.path.join(ROOT, "include", "sfmba.h")).read()
    body = re.search(r"typedef struct sfmba_triangulate_options \{(.*?)\} sfmba_triangulate_options;", header, re.S).group(1)
    fields = re.findall(r"^\s*(int32_t|double)\s+(\w+);", body, re.M)
    ctype = {"int32_t": ctypes.c_int32, "double": ctypes.c_double}
    assert [(name, ctype[t]) for t, name in fields] == list(T._fields_)
    assert ctypes.sizeof(T) == 40                                     # 2 int32, 4 doubles
    assert [getattr(T, n).offset for n, _ in T._fields_] == [0, 4, 8, 16, 24, 32]
    lib.sfmba_default_triangulate_options.argtypes = [ctypes.POINTER(T)]
    lib.sfmba_default_triangulate_options.restype = None

    class Guarded(ctypes.Structure):                                  # the library writes exactly sizeof(struct) bytes
        _fields_ = [("o", T), ("guard", ctypes.c_uint64)]
    g = Guarded()
    g.guard = 0xA5A5A5A5A5A5A5A5
    lib.sfmba_default_triangulate_options(ctypes.cast(ctypes.byref(g), ctypes.POINTER(T)))
    assert g.guard == 0xA5A5A5A5A5A5A5A5
    assert (g.o.max_iter, g.o.min_views, g.o.xtol, g.o.min_angle_deg, g.o.min_depth) == (10, 2, 1e-10, 1.0, 0.0)
    assert g.o.max_error_px == np.inf


def test_triangulate_points_rejects_a_matrix_that_is_no_rotation(cases):
    import sfmba
    K, M1, M2, p1, p2 = (cases[k] for k in ("K", "M1", "M2", "pts1", "pts2"))
    bad = M2.copy()
    bad[:, :3] = K @ (1.001 * np.linalg.solve(K, M2[:, :3]))         # K (1.001 R): scaled by 1e-3, far beyond 1e-6
    with pytest.raises(ValueError, match="rotation"):
        sfmba.triangulate_points(M1, bad, p1, p2, K)
    mirrored = M2.copy()
    mirrored[:, :3] = K @ (np.diag([1.0, 1.0, -1.0]) @ np.linalg.solve(K, M2[:, :3]))    # orthogonal, det = -1
    with pytest.raises(ValueError, match="rotation"):
        sfmba.triangulate_points(mirrored, M2, p1, p2, K)
    with pytest.raises(ValueError):
        sfmba.triangulate_points(M1[:, :3], M2, p1, p2, K)
    with pytest.raises(ValueError):
        sfmba.triangulate_points(M1, M2, p1, p2[:, :-1], K)


def test_camera_parameters_recovered_from_a_projection_matrix(cases):
    """K^-1 M -> (rotation vector, centre) -> K R [I | -T] gives M back: the route `triangulate_points` takes."""
    from sfmba import extras
    for key in ("M1", "M2"):
        cam = extras._cameras_from_projection(cases[key], cases["K"])
        assert np.allclose(cam, tr.cameras_from_projection(cases[key], cases["K"]), rtol=0, atol=1e-14)
        back = tr.projection_matrices(cam, 1, cases["K"])[0]
        assert np.abs(back - cases[key]).max() <= 1e-12 * np.abs(cases[key]).max()
