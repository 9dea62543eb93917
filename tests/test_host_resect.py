"""CPU-side checks of the resection feature: the numpy restatement (tests/resect_ref.py) against the reference's recorded
`_solve_pnp_linear` / `solve_pnp` output, the forty-sum form of A^T A against the explicit product, the scaling of the
linear translation, and the header / binding / built library.  No GPU compute is called here."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import resect_ref as rr

LIB = os.path.join(ROOT, "sfm-python_amd", "sfmba", "libsfmba.so")
EPS = np.finfo(np.float64).eps
BOUNDS = json.load(open(os.path.join(GOLDEN, "resect_bounds.json")))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__ as ge
        ge.build()
    return ctypes.CDLL(LIB)


@pytest.fixture(scope="module")
def cases():
    g = np.load(os.path.join(GOLDEN, "resect_cases.npz"), allow_pickle=False)
    out = []
    for k in range(len(g["n"])):
        sl = slice(int(g["ptr"][k]), int(g["ptr"][k + 1]))
        out.append(dict(n=int(g["n"][k]), noise=float(g["noise"][k]), X=g["X"][sl], uv=g["uv"][sl], K=g["K"],
                        rvec_true=g["rvec_true"][k], tvec_true=g["tvec_true"][k], R_lin=g["R_lin"][k], t_lin=g["t_lin"][k],
                        rvec=g["rvec"][k], tvec=g["tvec"][k], success=bool(g["success"][k])))
    return out


def test_fixture_is_data_of_the_expected_shape(cases):
    assert [(c["n"], c["noise"]) for c in cases] == [(n, z) for n in (6, 7, 12, 64, 257) for z in (0.0, 0.5)]
    assert [[c["n"], c["noise"]] for c in cases] == BOUNDS["cases"]
    for c in cases:
        assert c["X"].shape == (c["n"], 3) and c["uv"].shape == (c["n"], 2) and c["success"]
        assert c["R_lin"].shape == (3, 3) and c["rvec"].shape == (3,) and c["tvec"].shape == (3,)
    assert BOUNDS["factor"] == 100.0
    for key in ("linear_R_angle", "final_R_angle", "final_T_dist"):
        b = BOUNDS[key]
        assert b["measured_max"] == max(b["measured"]) and b["bound"] == BOUNDS["factor"] * b["measured_max"]


def test_restatement_matches_the_reference_on_every_case(cases):
    """Linear R against the reference's recorded R, the final pose against its recorded solve_pnp result: within the
    recorded bounds, and what this machine measures is what the generator recorded (to a factor 10)."""
    worst = dict(linear_R_angle=0.0, final_R_angle=0.0, final_T_dist=0.0)
    for c in cases:
        lin = rr.linear_pose(c["X"], c["uv"], c["K"])
        out = rr.resect_one(c["X"], c["uv"], c["K"])
        assert out["status"] == rr.OK and out["views"] == c["n"] and out["iters"] <= 6
        R_ref = rr.orc.rodrigues(c["rvec"])
        R, _ = rr.pose_from_params(out["params"])
        d = dict(linear_R_angle=rr.rotation_angle(c["R_lin"], lin["R"]), final_R_angle=rr.rotation_angle(R_ref, R),
                 final_T_dist=float(np.linalg.norm(-R_ref.T @ c["tvec"] - out["params"][3:])))
        for key, val in d.items():
            assert val <= BOUNDS[key]["bound"], (c["n"], c["noise"], key, val)
            worst[key] = max(worst[key], val)
        # the refinement never costs more than the linear pose
        assert rr.cost(out["params"], c["X"], c["uv"], c["K"]) <= rr.cost(out["linear"], c["X"], c["uv"], c["K"])
    for key, val in worst.items():
        print(f"{key}: {val:.3e} (recorded {BOUNDS[key]['measured_max']:.3e}, bound {BOUNDS[key]['bound']:.3e})")
        assert val <= 10 * BOUNDS[key]["measured_max"]


def test_forty_sums_give_the_explicit_product(cases):
    """A^T A assembled from S, S_u, S_v, S_w against A^T A of the explicit rows: entry by entry to the rounding of a sum
    of 2n terms, and the zero blocks exactly."""
    for c in cases:
        uvn = rr.normalise_pixels(c["uv"], c["K"])
        A = rr.dlt_rows(c["X"], uvn)
        full = A.T @ A
        mine = rr.ata_from_sums(rr.forty_sums(c["X"], uvn))
        assert np.array_equal(mine, mine.T) and not mine[0:4, 4:8].any() and not full[0:4, 4:8].any()
        mag = np.abs(A).T @ np.abs(A)
        assert np.all(np.abs(mine - full) <= 4 * c["n"] * EPS * mag), (c["n"], c["noise"])
        # the smallest eigenvector by Jacobi is the last right singular vector of A, to the conditioning of the pair
        lam = np.linalg.eigvalsh(full)
        lin = rr.linear_pose(c["X"], c["uv"], c["K"])
        v = np.linalg.svd(A)[2][-1]
        sin = np.linalg.norm(lin["h"] - v * (v @ lin["h"]))
        assert abs(np.linalg.norm(lin["h"]) - 1.0) <= 64 * EPS
        assert sin <= 64 * EPS * lam[-1] / (lam[1] - lam[0]), (c["n"], c["noise"], sin)


def test_jacobi_on_a_diagonal_and_against_eigh():
    d, V = rr.jacobi_eigh(np.diag(np.arange(12.0, 0.0, -1.0)), rr.SWEEPS12)
    assert np.array_equal(d, np.arange(12.0, 0.0, -1.0)) and np.array_equal(V, np.eye(12))
    rng = np.random.default_rng(8)
    for k in range(5):
        B = rng.normal(size=(30, 12)) * 10.0 ** rng.integers(-2, 3, 12)
        A = B.T @ B
        d, V = rr.jacobi_eigh(A, rr.SWEEPS12)
        assert np.abs(np.sort(d) - np.linalg.eigvalsh(A)).max() <= 64 * EPS * np.abs(d).max()
        assert np.abs(V.T @ V - np.eye(12)).max() <= 64 * EPS
        assert np.abs(V @ np.diag(d) @ V.T - A).max() <= 256 * EPS * np.abs(A).max()


def test_linear_translation_is_scaled(cases):
    """Exact data: t = m / (mean singular value of M) is the generating t to the conditioning of the linear system, where
    the reference's t = m of the unit-norm null vector is off by the order of |t| itself."""
    for c in cases:
        if c["noise"] != 0.0:
            continue
        lin = rr.linear_pose(c["X"], c["uv"], c["K"])
        lam = lin["eig"]
        tol = 32 * EPS * lam[-1] / lam[1] * max(1.0, np.linalg.norm(c["tvec_true"]))
        mine, theirs = np.linalg.norm(lin["t"] - c["tvec_true"]), np.linalg.norm(c["t_lin"] - c["tvec_true"])
        print(f"n={c['n']}: |t - t*| = {mine:.2e} (tolerance {tol:.2e}); the reference's linear t: {theirs:.2e}")
        assert mine <= tol and theirs > 0.1
        assert abs(np.linalg.det(lin["R"]) - 1.0) <= 64 * EPS and np.abs(lin["R"].T @ lin["R"] - np.eye(3)).max() <= 64 * EPS


def test_coplanar_points_are_degenerate_and_few_views_are_few():
    rng = np.random.default_rng(3)
    K = np.array([[2905.88, 0.0, 1416.0], [0.0, 2905.88, 1064.0], [0.0, 0.0, 1.0]])
    cam = np.stack([rng.uniform(-1, 1, 20), rng.uniform(-1, 1, 20), np.full(20, 6.0)], axis=1)     # a plane z = 6
    uv = cam @ K.T
    uv = uv[:, :2] / uv[:, 2:3]
    assert rr.resect_one(cam, uv, K)["status"] == rr.DEGENERATE
    assert rr.resect_one(cam[:5], uv[:5], K)["status"] == rr.FEW_VIEWS
    # from the pose in x the same plane is fine: the refinement needs no linear stage
    out = rr.resect_one(cam, uv, K, p0=np.array([0.01, -0.02, 0.01, 0.05, 0.0, -0.1]), start=1)
    assert out["status"] == rr.OK and np.abs(out["params"]).max() <= 1e-8


def test_header_binding_and_library_agree(lib):
    """The header declares the call, its option struct and which = 16; the binding lists them; a built library exports
    them and writes the documented defaults into exactly sizeof(struct) bytes."""
    from sfmba import _capi
    header = open(os.path.join(ROOT, "include", "sfmba.h")).read()
    assert re.search(r"\bint\s+sfmba_resect\(sfmba_handle\* h, const double\* x, const uint8_t\* cam_select", header)
    assert re.search(r"\bvoid\s+sfmba_default_resect_options\(sfmba_resect_options\* opt\);", header)
    assert re.search(r"\b16 k_resect of sfmba_resect", header)
    for name in ("sfmba_default_resect_options", "sfmba_resect"):
        assert name in _capi.SYMBOLS
        assert hasattr(lib, name), name
    T = _capi.ResectOptions
    body = re.search(r"typedef struct sfmba_resect_options \{(.*?)\} sfmba_resect_options;", header, re.S).group(1)
    fields = re.findall(r"^\s*(int32_t|double)\s+(\w+);", body, re.M)
    ctype = {"int32_t": ctypes.c_int32, "double": ctypes.c_double}
    assert [(name, ctype[t]) for t, name in fields] == list(T._fields_)
    assert ctypes.sizeof(T) == 40 and [getattr(T, n).offset for n, _ in T._fields_] == [0, 4, 8, 16, 24, 32]
    lib.sfmba_default_resect_options.argtypes = [ctypes.POINTER(T)]
    lib.sfmba_default_resect_options.restype = None

    class Guarded(ctypes.Structure):
        _fields_ = [("o", T), ("guard", ctypes.c_uint64)]
    g = Guarded()
    g.guard = 0xA5A5A5A5A5A5A5A5
    lib.sfmba_default_resect_options(ctypes.cast(ctypes.byref(g), ctypes.POINTER(T)))
    assert g.guard == 0xA5A5A5A5A5A5A5A5
    assert (g.o.max_iter, g.o.min_views, g.o.start, g.o.xtol, g.o.min_depth) == (20, 6, 0, 1e-10, 0.0)
    assert g.o.max_rms_px == np.inf


def test_solve_pnp_rejects_distortion_and_bad_shapes():
    import sfmba
    X, uv, K = np.zeros((6, 3)), np.zeros((6, 2)), np.eye(3)
    with pytest.raises(ValueError, match="distortion"):
        sfmba.solve_pnp(X, uv, K, dist=np.array([0.1, 0.0, 0.0, 0.0]))
    with pytest.raises(ValueError):
        sfmba.solve_pnp(X[:, :2], uv, K)
    with pytest.raises(ValueError):
        sfmba.solve_pnp(X, uv[:5], K)
