"""GPU tests of sfmba.reconstruct, the incremental loop on one back end.

The scene is a ring of ten cameras round 300 points, cut to one observation per (point, camera): 1920 observations, every
point seen twice or more.  The per-image feature lists are in shuffled row order; there is one match edge per image pair
u > v that shares points, with all shared points as pairs and E from the true relative pose; the first pair is (1, 0).

What is measured rather than derived -- how far the reconstruction's final cost is from that of the parent commit's
solver started at the truth, and how far its cameras and points are from that solve's after both were aligned to the
truth -- was measured once on the MI355X and is pinned with a tenfold margin in tests/golden/reconstruct_bounds.json
(the two runs stop on ftol at different iterates).  The measured cost difference itself must be below 1e-3: otherwise
the reconstruction did not reach the same minimum and the driver is wrong, not the bound."""
import json
import os

import numpy as np
import pytest

import plan_ref as pr
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

RADIUS = 8.0                                                     # of make_ring_problem
SCENE = dict(n_cameras=10, n_points=300, n_obs=3000, seed=3)


def bounds():
    return json.load(open(os.path.join(GOLDEN, "reconstruct_bounds.json")))


class Scene:
    """``corrupt``: (images, share, seed) -- that share of the images' features gets a pixel at least 50 px from the true
    one before the matches are built; ``starve``: (image, n) -- only n features of the image take part in the matches."""

    def __init__(self, corrupt=None, starve=None, params=SCENE):
        import sfmba
        from sfmba import api
        pb = sfmba.make_ring_problem(params["n_cameras"], params["n_points"], params["n_obs"], seed=params["seed"])
        self.pb, self.K = pb, pb.K
        C = pb.n_cameras
        ci, pi, uv = np.asarray(pb.camera_indices), np.asarray(pb.point_indices), np.asarray(pb.points_2d, dtype=np.float64)
        _, firsts = np.unique(pi * C + ci, return_index=True)
        firsts.sort()
        self.ci, self.pi, self.uv = ci[firsts], pi[firsts], uv[firsts].copy()
        rng = np.random.default_rng(8)
        self.feats = [rng.permutation(np.flatnonzero(self.ci == c)) for c in range(C)]      # image c: its observations, row by row
        self.row_of = np.empty(len(self.ci), dtype=np.int64)
        for f in self.feats:
            self.row_of[f] = np.arange(len(f))
        self.img_ptr = np.concatenate([[0], np.cumsum([len(f) for f in self.feats])]).astype(np.int64)
        self.obs_of_feat = np.concatenate(self.feats)                                       # global feature id -> observation
        self.corrupted = np.zeros(len(self.ci), dtype=bool)
        if corrupt is not None:
            images, share, seed = corrupt
            crng = np.random.default_rng(seed)
            for c in images:
                hit = crng.choice(self.feats[c], size=int(round(share * len(self.feats[c]))), replace=False)
                ang, far = crng.uniform(0.0, 2.0 * np.pi, len(hit)), crng.uniform(50.0, 200.0, len(hit))
                self.uv[hit] += np.stack([far * np.cos(ang), far * np.sin(ang)], axis=1)
                self.corrupted[hit] = True
        self.pts = [self.uv[f] for f in self.feats]
        matched = np.ones(len(self.ci), dtype=bool)
        if starve is not None:
            image, n = starve
            matched[self.feats[image][n:]] = False
        cams = pb.x_true[:6 * C].reshape(C, 6)
        Rm = [api._matrix_from_rotvec(cams[c, :3]) for c in range(C)]
        Kinv = np.linalg.inv(self.K)
        self.matches = []
        for u in range(C):
            for v in range(u):
                ou, ov = np.flatnonzero((self.ci == u) & matched), np.flatnonzero((self.ci == v) & matched)
                common, iu, iv = np.intersect1d(self.pi[ou], self.pi[ov], return_indices=True)
                if len(common) == 0:
                    continue
                pairs = np.stack([self.row_of[ou[iu]], self.row_of[ov[iv]]], axis=1)
                Rrel, trel = Rm[v] @ Rm[u].T, Rm[v] @ (cams[u, 3:] - cams[v, 3:])         # x_v = Rrel x_u + trel
                tx = np.array([[0.0, -trel[2], trel[1]], [trel[2], 0.0, -trel[0]], [-trel[1], trel[0], 0.0]])
                E = tx @ Rrel
                self.matches.append((u, v, pairs, Kinv.T @ E @ Kinv, E))

    def truth_for(self, rec):
        """x_true restricted to the reconstruction's final problem, and the original point of each of its points."""
        C = self.pb.n_cameras
        t = rec.tracks
        point_of_track = self.pi[self.obs_of_feat[t.track_feat[t.track_ptr[:-1]]]]
        cams = self.pb.x_true[:6 * C].reshape(C, 6)[rec.cam_of]
        pts = self.pb.x_true[6 * C:].reshape(-1, 3)[point_of_track[rec.pt_of]]
        return np.concatenate([cams.ravel(), pts.ravel()])


def similarity(src, dst):
    """s, R, t with dst ~ s R src + t in the least-squares sense (Umeyama)."""
    ms, md = src.mean(axis=0), dst.mean(axis=0)
    a, b = src - ms, dst - md
    U, S, Vt = np.linalg.svd(b.T @ a / len(src))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
    R = U @ D @ Vt
    s = np.trace(np.diag(S) @ D) / (a ** 2).sum() * len(src)
    return s, R, md - s * R @ ms


def aligned(x, n_cameras, true_centres):
    """Camera centres and points of x after the similarity that takes its centres to the true ones."""
    cams, pts = x[:6 * n_cameras].reshape(-1, 6), x[6 * n_cameras:].reshape(-1, 3)
    s, R, t = similarity(cams[:, 3:], true_centres)
    return s * cams[:, 3:] @ R.T + t, s * pts @ R.T + t


def measure(be, scene, rec):
    """-> dict: the final cost of the reconstruction against the cost of sfmba.least_squares started from the truth on
    the same observation set, relative to the latter, and the worst centre / point distance between the two results
    after both were aligned to the true centres, relative to the ring radius."""
    import sfmba
    x, args = rec.problem()
    n_cameras = args[0]
    be.set_fixed_cameras(())
    be.set_problem(*args)
    cost = 0.5 * float(np.sum(be.residuals(x) ** 2))
    x_truth = scene.truth_for(rec)
    ref = sfmba.least_squares(sfmba.compute_residuals, x_truth, x_scale="jac", ftol=1e-10, method="trf", args=args, backend=be)
    centres = x_truth[:6 * n_cameras].reshape(-1, 6)[:, 3:]
    ca, pa = aligned(x, n_cameras, centres)
    cb, pb_ = aligned(ref.x, n_cameras, centres)
    return dict(cost=cost, cost_ref=float(ref.cost), cost_rel=abs(cost - float(ref.cost)) / float(ref.cost),
                centre_rel=float(np.linalg.norm(ca - cb, axis=1).max() / RADIUS),
                point_rel=float(np.linalg.norm(pa - pb_, axis=1).max() / RADIUS),
                centre_vs_truth_rel=float(np.linalg.norm(ca - centres, axis=1).max() / RADIUS))


@pytest.fixture(scope="module")
def be():
    import sfmba
    b = sfmba.Backend(0)
    yield b
    b.close()


@pytest.fixture(scope="module")
def clean():
    return Scene()


def check_against_bounds(m, b):
    print({k: f"{v:.3e}" for k, v in m.items()})
    assert b["clean"]["cost_rel"] < 1e-3                          # the measured value itself
    assert m["cost_rel"] <= 10.0 * b["clean"]["cost_rel"]
    assert m["centre_rel"] <= 10.0 * b["clean"]["centre_rel"] and m["point_rel"] <= 10.0 * b["clean"]["point_rel"]


def test_the_scene_is_the_one_the_bounds_were_measured_on(clean):
    b = bounds()
    assert b["scene"] == SCENE and b["radius"] == RADIUS
    assert len(clean.ci) == 1920 and int((np.bincount(clean.pi, minlength=300) >= 2).sum()) == 300
    assert len(clean.matches) == 45


def test_clean_run_one_image_per_round(be, clean):
    import sfmba
    rec = sfmba.reconstruct(clean.matches, clean.pts, clean.K, init=(1, 0), batch=1, backend=be, record_state=True)
    assert rec.tracks.n_tracks == 300 and rec.tracks.counts["observations"] == 1920
    assert rec.registered.all() and np.isfinite(rec.cameras).all()
    assert rec.known.sum() >= 0.95 * 300
    assert np.isfinite(rec.points[rec.known]).all() and np.isnan(rec.points[~rec.known]).all()
    assert len(rec.rounds) == 8
    for k, info in enumerate(rec.rounds):
        v = pr.plan_views_ref(rec.tracks, info["registered_before"], info["known_before"])
        if k == 0:
            assert info["registered_before"].tolist() == [True, True] + [False] * 8 and info["known_before"].sum() == 114
        left = np.flatnonzero(~info["registered_before"])
        predicted = int(left[np.argmax(v["img_known"][left])])                          # (argmax: the first, the lower id)
        assert v["img_known"][predicted] >= 79
        assert info["tried"] == [predicted] and info["registered"] == [predicted] and not info["failed"], k
        assert info["n_obs"] > 0 and info["rmse_after"] <= info["rmse_before"]
    check_against_bounds(measure(be, clean, rec), bounds())


def test_clean_run_all_images_in_one_round(be, clean):
    import sfmba
    rec = sfmba.reconstruct(clean.matches, clean.pts, clean.K, init=(1, 0), batch=0, backend=be)
    assert rec.registered.all() and rec.known.sum() >= 0.95 * 300
    assert len(rec.rounds) == 1 and sorted(rec.rounds[0]["registered"]) == list(range(2, 10))
    check_against_bounds(measure(be, clean, rec), bounds())


def test_wrong_matches_are_filtered(be):
    import sfmba
    scene = Scene(corrupt=((2, 5, 7), 0.10, 11))
    assert scene.corrupted.sum() == sum(int(round(0.1 * len(scene.feats[c]))) for c in (2, 5, 7))
    rec = sfmba.reconstruct(scene.matches, scene.pts, scene.K, init=(1, 0), batch=1, backend=be, filter=True,
                            filter_options=dict(max_error_px=4.0))
    assert rec.registered.all()
    x, args = rec.problem()
    be.set_fixed_cameras(())
    be.set_problem(*args)
    st = be.reprojection_stats(x, want=("obs",))
    assert st.obs_err.max() <= 4.0                               # the driver's contract
    in_final = np.zeros(len(scene.ci), dtype=bool)
    in_final[scene.obs_of_feat[rec.obs_feat]] = True
    print(f"corrupted observations dropped: {int((scene.corrupted & ~in_final).sum())} of {int(scene.corrupted.sum())}; "
          f"clean observations dropped: {int((~scene.corrupted & ~in_final).sum())} of {int((~scene.corrupted).sum())}")
    m, b = measure(be, scene, rec), bounds()
    print({k: f"{v:.3e}" for k, v in m.items()})
    # the clean run's pinned bound times the ratio of the two runs' distances as measured (wrong_matches.centre_rel is on record)
    assert m["centre_rel"] <= 10.0 * b["clean"]["centre_rel"] * b["wrong_matches"]["ratio"]


def test_a_camera_that_cannot_register(be):
    import sfmba
    scene = Scene(starve=(9, 5))
    rec = sfmba.reconstruct(scene.matches, scene.pts, scene.K, init=(1, 0), batch=1, backend=be)
    assert rec.registered.tolist() == [True] * 9 + [False] and np.isnan(rec.cameras[9]).all()
    closing = rec.rounds[-1]
    assert closing["tried"] == [] and closing["failed"] == {9: "few_known"}
    assert len(rec.rounds) == 8 and all(len(r["registered"]) == 1 for r in rec.rounds[:-1])
    assert 9 not in rec.cam_of


def test_given_tracks_a_held_first_camera_and_a_chosen_first_pair(be, clean):
    import sfmba
    tracks = sfmba.build_tracks(clean.matches, [len(p) for p in clean.pts], backend=be)
    rec = sfmba.reconstruct(clean.matches, clean.pts, clean.K, tracks=tracks, init=(1, 0), batch=2, fix_first=True, backend=be)
    assert rec.tracks is tracks and rec.registered.all() and rec.known.sum() >= 0.95 * 300
    assert not rec.cameras[1].any()                              # held in every solve: still at the identity, to the bit
    assert [len(r["tried"]) for r in rec.rounds] == [2, 2, 2, 2]
    # The same minimum in another gauge (a held camera removes six of the seven gauge freedoms, not a residual).  Both
    # solves stop when a step lowers the cost by less than ftol = 1e-10 of it; 1e-6 leaves four orders for the steps
    # that were not taken, and is three orders below the issue's own "did not reach the same minimum" mark of 1e-3.
    m = measure(be, clean, rec)
    print({k: f"{v:.3e}" for k, v in m.items()})
    assert m["cost_rel"] < 1e-6
    other = sfmba.Backend(0)
    try:
        with pytest.raises(ValueError):                          # tracks that this back end did not build
            sfmba.reconstruct(clean.matches, clean.pts, clean.K, tracks=tracks, init=(1, 0), backend=other)
        with pytest.raises(ValueError):
            sfmba.reconstruct(clean.matches, clean.pts, clean.K, init=(1, 1), backend=other)
    finally:
        other.close()
    # init=None: the first pair by select_initial_pair over the edges
    rec = sfmba.reconstruct(clean.matches, clean.pts, clean.K, batch=0, backend=be)
    assert rec.registered.all() and rec.known.sum() >= 0.95 * 300
