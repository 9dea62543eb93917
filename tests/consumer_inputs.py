"""Inputs that several tests of the consumers (statistics, triangulation, resection) and tools/ab_consumer_bits.py share."""
import numpy as np

from oracle import ba_oracle as orc

from kernel_source import kernel_constant


def ring_tracks(n_cameras, n_tracks, special, cam_seed, seed):
    """Cameras on a ring (make_ring_problem), tracks of three and four views in point-major order, among them tracks of
    exactly special[p] views; pixels are the projections plus 0.5 px of noise.  -> (x, args)."""
    import sfmba
    base = sfmba.make_ring_problem(n_cameras, 50, 400, seed=cam_seed)
    C, K = n_cameras, base.K
    cams = base.x_true[:6 * C].reshape(C, 6)
    rng = np.random.default_rng(seed)
    P = n_tracks
    lengths = np.where(np.arange(P) % 2 == 0, 3, 4)
    for p, n in special.items():
        lengths[p] = n
    pts = rng.normal(0.0, 1.0, (P, 3))
    ci = np.concatenate([rng.permutation(C)[:n] for n in lengths]).astype(np.int64)
    pi = np.repeat(np.arange(P, dtype=np.int64), lengths)
    x = np.concatenate([cams.ravel(), pts.ravel()])
    proj = orc.compute_residuals(x, C, P, ci, pi, np.zeros((len(ci), 2)), K).reshape(-1, 2)
    uv = proj + rng.normal(0.0, 0.5, proj.shape)
    return x, (C, P, ci, pi, uv, K)


# runs of more than one 64-observation block of the wave form: one block less one, one block, one block and one
# observation, two blocks, two blocks and two
LONG_RUNS = {20: 63, 21: 64, 90: 65, 130: 128, 204: 130}


def long_run_problem():
    """136 cameras on a ring, 205 tracks of 3-4 views, among them the LONG_RUNS (1147 observations).  -> (x, args)"""
    return ring_tracks(136, 205, LONG_RUNS, cam_seed=4, seed=23)


def point_interleaved_order(pi):
    """A non-point-major order of the observations that keeps the order inside every run (first observation of every
    point, then the second, ...): the stored order, and with it every sum, is that of the point-major problem."""
    pos = np.arange(len(pi)) - np.searchsorted(pi, pi)
    return np.lexsort((pi, pos))


def boundary_problem(seed=11):
    """A few thousand points of 2-3 views (runs that straddle the 64-observation tiles and the 1024-observation
    workgroups of the per-observation sweep, and the 256-point workgroups of the reduction), three runs of exactly
    L - 1, L and L + 1 views around the long-track switch-over L, in point-major order.  -> (x, args)"""
    L, tile, block = kernel_constant("kStatsLongTrack"), 64, kernel_constant("kSweepThreads")
    rng = np.random.default_rng(seed)
    C = L + 8
    lens = rng.integers(2, 4, 4000)
    for k, n in ((700, L - 1), (701, L), (2900, L + 1), (3999, L)):      # (701 follows 700 in one wave; 3999: the last point)
        lens[k] = n
    P = len(lens)
    ptr = np.concatenate([[0], np.cumsum(lens)])
    # runs must straddle tile and workgroup boundaries
    inside = lambda m: np.any((ptr[:-1] % m != 0) & (ptr[:-1] // m != (ptr[1:] - 1) // m))
    assert inside(tile) and inside(block)
    pi = np.repeat(np.arange(P, dtype=np.int64), lens)
    ci = np.concatenate([rng.permutation(C)[:n] for n in lens]).astype(np.int64)     # distinct cameras inside a run
    w = rng.normal(0.0, 0.1, (C, 3))
    T = rng.normal(0.0, 0.5, (C, 3))
    X = rng.normal(0.0, 1.0, (P, 3)) + [0.0, 0.0, 10.0]
    from sfmba import K_SCEAUX
    from sfmba.synthetic import _rodrigues_batch
    q = np.einsum("nij,nj->ni", _rodrigues_batch(w)[ci], X[pi] - T[ci]) @ K_SCEAUX.T
    uv = q[:, :2] / q[:, 2:3] + rng.normal(0.0, 0.7, (len(ci), 2))
    x = np.concatenate([np.hstack([w, T]).ravel(), X.ravel()])
    return x, (C, P, ci, pi, uv, K_SCEAUX.copy())


def camera_slices_problem(lengths, seed=31):
    """One camera per entry of `lengths` with that many points of its own 4..9 units in front of it, 0.5 px of noise
    (camera slices at the edges of k_resect's strided loop); the cameras of x are the true ones, slightly turned and
    moved.  -> (x, args)"""
    from sfmba import K_SCEAUX
    rng = np.random.default_rng(seed)
    C = len(lengths)
    w = rng.normal(0.0, 0.3, (C, 3))
    T = rng.normal(0.0, 1.5, (C, 3))
    ci = np.repeat(np.arange(C, dtype=np.int64), lengths)
    pi = np.arange(len(ci), dtype=np.int64)
    cam = np.stack([rng.uniform(-1.8, 1.8, len(ci)), rng.uniform(-1.3, 1.3, len(ci)), rng.uniform(4.0, 9.0, len(ci))], axis=1)
    q = cam @ K_SCEAUX.T
    uv = q[:, :2] / q[:, 2:3] + rng.normal(0.0, 0.5, (len(ci), 2))
    X = np.einsum("nji,nj->ni", orc.rodrigues(w)[ci], cam) + T[ci]                 # X = R^T cam + T
    x = np.concatenate([(np.hstack([w, T]) + rng.normal(0.0, 0.01, (C, 6))).ravel(), X.ravel()])
    return x, (C, len(pi), ci, pi, uv, K_SCEAUX.copy())
