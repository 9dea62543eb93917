"""What a handle did before must not change what a call returns now: the catalogue of calls, the pasts and the problem
sequences that tests/test_gpu_history.py runs on a device and tests/test_host_history.py checks without one (DESIGN.md
section 31).

Nothing here needs a device to be imported or to build its inputs.  Every entry of `ENTRIES` is a function
``(backend, inputs) -> dict of outputs``; ``inputs`` is `inputs(scale)`, one set of arguments for every stage at one of
four scales: "entry" (what the call under test is given), "twin" (the same sizes in every dimension a buffer, a stride or
a cache key depends on, other content), "larger" and "smaller" (every such dimension strictly larger / smaller).  An
entry sets the state it reads (problem, descriptors, tracks) itself, so it means the same on a fresh handle and on a
used one; it never touches a sticky setting (precision, held cameras, debug options): the pasts put those back.

The inputs come from the builders the stage modules use: `sfmba.make_problem`, `consumer_inputs.ring_tracks` and
`camera_slices_problem`, the grid of `covariance_ref`, the scenes of the pair models' restatements,
`track_ref.Scene` and `plan_ref.pixels`."""
import functools

import numpy as np

import covariance_ref
import essential_ref
import homography_ref
import plan_ref
import similarity_ref
import track_ref
import two_view_ref
from consumer_inputs import camera_slices_problem, ring_tracks
from kernel_source import kernel_constant

SCALES = ("entry", "twin", "larger", "smaller")
LONG = kernel_constant("kStatsLongTrack")                      # the lane / wave switch-over of every per-track walk
CAM_STRIDE = kernel_constant("kCamThreads")                    # one stride of a camera slice
PAIR_LDS, SIM_LDS = kernel_constant("kTwoViewLdsPairs"), kernel_constant("kSimLdsPairs")
PAIR_SLICE, SIM_SLICE, PNP_SLICE = (kernel_constant(k) for k in ("kTwoViewMinSlice", "kSimMinSlice", "kPnpMinSlice"))
K_PIX = np.array([[2905.88, 0.0, 1416.0], [0.0, 2905.88, 1064.0], [0.0, 0.0, 1.0]])
TIMING = ("kernel_us",)

# ---- the sizes -------------------------------------------------------------------------------------------------------------
# One row per scale.  "twin" repeats "entry" with other seeds.  Everything that sizes a buffer grows from "smaller" to
# "entry" to "larger"; tests/test_host_history.py holds that, and that the entry sizes sit on both sides of the switches.
SIZES = {
    "entry": dict(
        seed=100,
        ba=(26, 150, 1300),                                                     # C > 21: the PCG path, not the dense one
        tracks=dict(C=40, P=60, special={5: LONG - 1, 6: LONG, 20: LONG + 1, 41: 40}), tri_H=24,
        slices=[7, 40, CAM_STRIDE + 1, CAM_STRIDE + 44, 12], pnp_H=PNP_SLICE + 32,
        cov=dict(C=8, mult=[1, 2, 4, 9, 1, 3, 4, 9]),                           # runs of 7, 14, 32 (the switch), 72, 7, 21, 32, 72
        pairs=[20, 150, PAIR_LDS + 4], pair_H=PAIR_SLICE * 6, sim=[10, 120, SIM_LDS + 28], sim_H=SIM_SLICE + 32,
        descs=[70, 130, 65, 40], match_edges=[(1, 0), (2, 1), (3, 0), (0, 2)],
        images=40, paths=[2, 3, LONG - 1, LONG, LONG + 1, 40, 5, 4, 2, 7], loose=6),
    "larger": dict(
        seed=300,
        ba=(34, 300, 2600),
        tracks=dict(C=48, P=150, special={5: LONG - 1, 6: LONG, 20: LONG + 1, 41: 48, 70: 47}), tri_H=40,
        slices=[9, 50, CAM_STRIDE + 14, CAM_STRIDE + 74, 20, 130], pnp_H=PNP_SLICE + 96,
        cov=dict(C=10, mult=[1, 2, 4, 9, 1, 3, 4, 9, 3, 5, 6, 8]),
        pairs=[30, 200, PAIR_LDS + 104, 60], pair_H=PAIR_SLICE * 10, sim=[14, 160, SIM_LDS + 128, 40], sim_H=SIM_SLICE + 96,
        descs=[90, 150, 80, 60, 50], match_edges=[(1, 0), (2, 1), (3, 0), (0, 2), (4, 1), (2, 4)],
        images=48, paths=[2, 3, LONG - 1, LONG, LONG + 1, 40, 5, 4, 2, 7, 48, 20, 35, 6], loose=9),
    "smaller": dict(
        seed=400,
        ba=(23, 60, 500),
        tracks=dict(C=34, P=30, special={5: LONG - 1, 6: LONG, 20: LONG + 1}), tri_H=10,
        slices=[7, 30, 100, 8], pnp_H=32,
        cov=dict(C=6, mult=[1, 2, 6, 3]),
        pairs=[12, 100], pair_H=PAIR_SLICE * 2, sim=[8, 90], sim_H=SIM_SLICE - 24,
        descs=[40, 60, 30], match_edges=[(1, 0), (2, 1), (0, 2)],
        images=34, paths=[2, 3, LONG - 1, LONG, LONG + 1], loose=3),
}
SIZES["twin"] = dict(SIZES["entry"], seed=200)


def mask(seed, n, share):
    """A boolean mask of n entries, about `share` of them set, never empty."""
    m = np.random.default_rng(seed).random(n) < share
    if n and not m.any():
        m[0] = True
    return m


def positions(seed, used, H, S):
    """(len(used), H, S) int32 sample positions, each among the `used[k]` used members of its group."""
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(0, max(int(n), S), (H, S)) for n in used]).astype(np.int32)


def used_per_group(ptr, use):
    return np.add.reduceat(use.astype(np.int64), ptr[:-1]) if len(ptr) > 1 else np.zeros(0, np.int64)


def shuffled_slices(lengths, seed):
    """`camera_slices_problem` with its observations in a random order and the points renumbered in that order: still
    point-major (every point is seen once), but the camera-major permutation is no identity and differs per seed."""
    x, (C, P, ci, pi, uv, K) = camera_slices_problem(lengths, seed=seed)
    o = np.random.default_rng(seed + 1).permutation(len(ci))
    X = x[6 * C:].reshape(P, 3)[pi[o]]
    return np.concatenate([x[:6 * C], X.ravel()]), (C, P, np.ascontiguousarray(ci[o]), np.arange(P, dtype=np.int64),
                                                   np.ascontiguousarray(uv[o]), K)


def cov_grid(C, mult, seed):
    """The grid of covariance_ref's "grid21_multi" at any size: point p is seen `mult[p]` rounds, each round by the
    cameras in an order of the seed's and each time with a pixel of its own (0.5 px of noise); in the points of up to
    three rounds every round leaves one camera of the seed's out, so the cameras of two seeds see other points, at equal N."""
    import sfmba
    from oracle import ba_oracle as orc
    rng = np.random.default_rng(seed)
    P = len(mult)
    pb = sfmba.make_problem(C, max(P, 12), C * max(P, 12), seed=seed)
    runs = [np.concatenate([rng.permutation(C)[:C - (1 if m <= 3 else 0)] for _ in range(m)]).astype(np.int64) for m in mult]
    ci = np.concatenate(runs)
    pi = np.repeat(np.arange(P, dtype=np.int64), [len(r) for r in runs])
    x = np.concatenate([pb.x_true[:6 * C], pb.x_true[6 * pb.n_cameras:6 * pb.n_cameras + 3 * P]])
    proj = orc.compute_residuals(x, C, P, ci, pi, np.zeros((len(ci), 2)), pb.K).reshape(-1, 2)
    return x, (C, P, ci, pi, proj + rng.normal(0.0, 0.5, proj.shape), pb.K)


def edge_batch(edges):
    ptr = np.concatenate([[0], np.cumsum([len(e[0]) for e in edges])]).astype(np.int64)
    return np.concatenate([e[0] for e in edges]), np.concatenate([e[1] for e in edges]), ptr


def pair_inputs(kind, counts, H, S, seed):
    """A batch of one model: pts1, pts2, ptr, a mask, samples among the used pairs, and what the model needs besides."""
    rng = np.random.default_rng(seed)
    extra = {}
    if kind == "fundamental":
        edges = [two_view_ref.make_pairs(rng, n, K_PIX, noise=0.5, outliers=0.2) for n in counts]
    elif kind == "homography":
        edges = [homography_ref.planar_pairs(rng, n, K_PIX, noise=0.5, outliers=0.2) for n in counts]
    elif kind == "essential":
        edges = [essential_ref.scene(rng, n, essential_ref.K_TEST, noise=0.5, outliers=0.2) for n in counts]
        extra["K"] = essential_ref.K_TEST
    elif kind == "similarity":
        edges = [similarity_ref.similar_sets(rng, n, noise=0.01, outliers=0.2) for n in counts]
    elif kind == "pose":
        edges = [two_view_ref.make_pairs(rng, n, K_PIX, noise=0.5, outliers=0.1) for n in counts]
        extra["K"] = K_PIX
        extra["E"] = np.stack([two_view_ref.essential_from_pose(e[2], e[3]) for e in edges])
    a, b, ptr = edge_batch(edges)
    use = mask(seed + 1, len(a), 0.8)
    return dict(a=a, b=b, ptr=ptr, use=use, H=H, samples=positions(seed + 2, used_per_group(ptr, use), H, S), **extra)


def track_scene(n_images, paths, loose, seed):
    """Paths of the given lengths from image 0 on, in an order and a direction of the seed's, and `loose` features in no
    pair; the sizes (images, features, edges, pairs, tracks) depend on the lengths alone."""
    rng = np.random.default_rng(seed)
    sc = track_ref.Scene(n_images)
    for k in rng.permutation(len(paths)):
        sc.path(int(paths[k]), descending=bool(rng.integers(0, 2)))
    for _ in range(loose):
        sc.feature(int(rng.integers(0, n_images)))
    return sc.batch()


@functools.lru_cache(maxsize=None)
def inputs(scale):
    """The arguments of every stage at one scale (built once)."""
    import sfmba
    z = SIZES[scale]
    s = z["seed"]
    I = dict(scale=scale, seed=s)
    I["ba"] = sfmba.make_problem(*z["ba"], seed=s)
    rng = np.random.default_rng(s + 1)
    C, P, _ = z["ba"]
    I["ba_vec"] = dict(dc=rng.uniform(1.0, 20.0, 6 * C), dp=rng.uniform(1.0, 20.0, 3 * P), v=rng.normal(size=6 * C))
    t = z["tracks"]
    x, args = ring_tracks(t["C"], t["P"], t["special"], cam_seed=s + 2, seed=s + 3)
    I["tracks"] = dict(x=x, args=args, select=mask(s + 4, args[1], 0.7), use=mask(s + 5, len(args[2]), 0.85), H=z["tri_H"])
    x, args = shuffled_slices(z["slices"], s + 6)
    use = mask(s + 7, len(args[2]), 0.85)
    used = np.bincount(args[2][use], minlength=args[0])
    I["slices"] = dict(x=x, args=args, select=mask(s + 8, args[0], 0.7), use=use, H=z["pnp_H"],
                       samples=positions(s + 9, used, z["pnp_H"], 3))
    x, args = cov_grid(z["cov"]["C"], z["cov"]["mult"], s + 10)
    I["cov"] = dict(x=x, args=args)
    for k, kind in enumerate(("fundamental", "homography", "essential", "pose")):
        I[kind] = pair_inputs(kind, z["pairs"], z["pair_H"], {"fundamental": 8, "homography": 4, "essential": 5, "pose": 1}[kind],
                              s + 20 + 3 * k)
    I["similarity"] = pair_inputs("similarity", z["sim"], z["sim_H"], 3, s + 40)
    rng = np.random.default_rng(s + 50)
    I["descs"] = [rng.integers(0, 256, size=(n, 128)).astype(np.uint8) for n in z["descs"]]
    I["match_edges"] = np.array(z["match_edges"], dtype=np.int32)
    batch = track_scene(z["images"], z["paths"], z["loose"], s + 60)
    I["trk"] = dict(batch=batch, use=mask(s + 61, len(batch[3]), 0.9), kp=plan_ref.pixels(np.random.default_rng(s + 62), batch[0]))
    return I


def dims(scale):
    """Every dimension that sizes a buffer, a stride or a cache key, by name."""
    I = inputs(scale)
    d = {}
    for name in ("tracks", "slices", "cov"):
        C, P, ci = I[name]["args"][0], I[name]["args"][1], I[name]["args"][2]
        d.update({f"{name}.C": C, f"{name}.P": P, f"{name}.N": len(ci), f"{name}.ld": (len(ci) + 255) // 256 * 256})
    pb = I["ba"]
    d.update({"ba.C": pb.n_cameras, "ba.P": pb.n_points, "ba.N": pb.n_obs, "ba.ld": (pb.n_obs + 255) // 256 * 256})
    d["tracks.H"], d["slices.H"] = I["tracks"]["H"], I["slices"]["H"]
    for kind in ("fundamental", "homography", "essential", "pose", "similarity"):
        d.update({f"{kind}.edges": len(I[kind]["ptr"]) - 1, f"{kind}.pairs": len(I[kind]["a"]), f"{kind}.H": I[kind]["H"]})
    d.update({"descs.images": len(I["descs"]), "descs.rows": sum(len(a) for a in I["descs"]), "descs.dim": I["descs"][0].shape[1],
              "descs.dtype": str(I["descs"][0].dtype), "match.edges": len(I["match_edges"])})
    img_ptr, edges, pair_ptr, pairs = I["trk"]["batch"]
    t = track_ref.build_tracks_ref(img_ptr, edges, pair_ptr, pairs, conflicts=1)
    d.update({"trk.images": len(img_ptr) - 1, "trk.features": int(img_ptr[-1]), "trk.edges": len(edges), "trk.pairs": len(pairs),
              "trk.tracks": len(t["track_ptr"]) - 1})
    return d


# ---- outputs -----------------------------------------------------------------------------------------------------------------
def outputs_of(obj):
    """Every array and scalar of a result object or dict but the timing fields, as arrays by name."""
    out = {}
    for name, v in (obj.items() if isinstance(obj, dict) else vars(obj).items()):
        if name in TIMING or v is None:
            continue
        if isinstance(v, dict):
            out.update({f"{name}.{k}": np.asarray(w) for k, w in v.items()})
        else:
            out[name] = np.asarray(v)
    return out


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def differing(got, want):
    """The names of the outputs that are not the same bytes (a missing or an extra name counts)."""
    return sorted(k for k in set(got) | set(want) if k not in got or k not in want or not same(got[k], want[k]))


RESULT_FIELDS = ("cost", "cost0", "optimality", "rmse", "rmse0", "nfev", "njev", "iterations", "pcg_iterations", "status",
                 "last_step_norm", "last_reg")


def solve_outputs(be, x0, max_nfev=12):
    opt = be.default_options()
    opt.ftol, opt.max_nfev = 1e-10, max_nfev
    x, res, fun, grad = be.solve(x0, opt)
    out = {name: np.asarray(getattr(res, name)) for name in RESULT_FIELDS}
    out.update(x=x, fun=fun, grad=grad, pcg_history=np.asarray(be.pcg_history(), dtype=np.int64))
    return out


def named(names, arrays):
    return dict(zip(names, arrays))


# The solver entries, once: (backend, x, the vectors of `vectors`, max_nfev) -> outputs.  The catalogue entries and the
# sequences both go through this table.
SOLVER_CALLS = {
    "residuals": lambda be, x, v, n: dict(r=be.residuals(x)),
    "residual_jacobian": lambda be, x, v, n: named(("r", "Jc", "Jp"), be.residual_jacobian(x)),
    "normal_blocks": lambda be, x, v, n: named(("U", "V", "gc", "gp"), be.normal_blocks(x)),
    "schur_matvec": lambda be, x, v, n: dict(y=be.schur_matvec(x, v["dc"], v["dp"], v["v"])),
    "rhs_precond": lambda be, x, v, n: named(("rhs", "sd", "minv"), be.rhs_precond(x, v["dc"], v["dp"])),
    "solve": lambda be, x, v, n: solve_outputs(be, x, n),
}


def solver_outputs(be, x, vec, max_nfev=12):
    """Every solver entry at x on the problem the handle holds -> {entry: outputs}."""
    return {name: call(be, x, vec, max_nfev) for name, call in SOLVER_CALLS.items()}


# ---- the catalogue --------------------------------------------------------------------------------------------------------------
ENTRIES = {}            # name -> dict(fn, reads, calls, masked)


def entry(name, reads, calls, masked=None):
    """Register `fn(be, I)`.  reads: the handle state it depends on; calls: the C functions it reaches; masked: the name
    of the variant with every mask and optional output (None: this is it, or the call has none)."""
    def deco(fn):
        ENTRIES[name] = dict(fn=fn, reads=reads, calls=calls, masked=masked or name)
        return fn
    return deco


def _solver(name, calls):
    @entry(name, ("problem",), ("sfmba_set_problem_i64",) + calls)
    def fn(be, I, name=name):
        be.set_problem(*I["ba"].args)
        return SOLVER_CALLS[name](be, I["ba"].x0, I["ba_vec"], 12)


for _name, _calls in (("residuals", ("sfmba_residuals",)), ("residual_jacobian", ("sfmba_residual_jacobian",)),
                      ("normal_blocks", ("sfmba_normal_blocks",)), ("schur_matvec", ("sfmba_schur_matvec",)),
                      ("rhs_precond", ("sfmba_rhs_precond",)),
                      ("solve", ("sfmba_solve_from", "sfmba_get_fun_grad", "sfmba_get_pcg_history"))):
    _solver(_name, _calls)


@entry("reprojection_stats", ("problem",), ("sfmba_set_problem", "sfmba_reprojection_stats"), masked="reprojection_stats_filtered")
def _(be, I):
    be.set_problem(*I["tracks"]["args"])
    return outputs_of(be.reprojection_stats(I["tracks"]["x"]))


@entry("reprojection_stats_filtered", ("problem",), ("sfmba_set_problem", "sfmba_reprojection_stats"))
def _(be, I):
    be.set_problem(*I["tracks"]["args"])
    return outputs_of(be.reprojection_stats(I["tracks"]["x"], max_error_px=1.2, min_depth=0.5, min_angle_deg=2.0, min_views=3))


@entry("triangulate", ("problem",), ("sfmba_set_problem", "sfmba_triangulate"), masked="triangulate_masked")
def _(be, I):
    be.set_problem(*I["tracks"]["args"])
    return outputs_of(be.triangulate(I["tracks"]["x"]))


@entry("triangulate_masked", ("problem",), ("sfmba_set_problem", "sfmba_triangulate"))
def _(be, I):
    t = I["tracks"]
    be.set_problem(*t["args"])
    return outputs_of(be.triangulate(t["x"], select=t["select"], obs_use=t["use"]))


@entry("triangulate_ransac", ("problem",), ("sfmba_set_problem", "sfmba_triangulate_ransac"), masked="triangulate_ransac_masked")
def _(be, I):
    t = I["tracks"]
    be.set_problem(*t["args"])
    return outputs_of(be.triangulate_ransac(t["x"], max_pairs=t["H"], seed=11))


@entry("triangulate_ransac_masked", ("problem",), ("sfmba_set_problem", "sfmba_triangulate_ransac"))
def _(be, I):
    t = I["tracks"]
    be.set_problem(*t["args"])
    return outputs_of(be.triangulate_ransac(t["x"], select=t["select"], obs_use=t["use"], want_hyp=True, max_pairs=t["H"], seed=11))


@entry("resect", ("problem",), ("sfmba_set_problem", "sfmba_resect"), masked="resect_masked")
def _(be, I):
    be.set_problem(*I["slices"]["args"])
    return outputs_of(be.resect(I["slices"]["x"]))


@entry("resect_masked", ("problem",), ("sfmba_set_problem", "sfmba_resect"))
def _(be, I):
    c = I["slices"]
    be.set_problem(*c["args"])
    return outputs_of(be.resect(c["x"], select=c["select"], obs_use=c["use"]))


@entry("resect_ransac", ("problem",), ("sfmba_set_problem", "sfmba_resect_ransac"), masked="resect_ransac_masked")
def _(be, I):
    c = I["slices"]
    be.set_problem(*c["args"])
    return outputs_of(be.resect_ransac(c["x"], max_iters=c["H"], seed=7, threshold=3.0))


@entry("resect_ransac_masked", ("problem",), ("sfmba_set_problem", "sfmba_resect_ransac"))
def _(be, I):
    c = I["slices"]
    be.set_problem(*c["args"])
    return outputs_of(be.resect_ransac(c["x"], select=c["select"], obs_use=c["use"], samples=c["samples"], want_hyp=True, threshold=3.0))


@entry("covariance_marginal", ("problem",), ("sfmba_set_problem", "sfmba_covariance"))
def _(be, I):
    be.set_problem(*I["cov"]["args"])
    return outputs_of(be.covariance(I["cov"]["x"], kind="marginal", want_full=True))


@entry("covariance_conditional", ("problem",), ("sfmba_set_problem", "sfmba_covariance"))
def _(be, I):
    be.set_problem(*I["cov"]["args"])
    return outputs_of(be.covariance(I["cov"]["x"], kind="conditional"))


PAIR_CALL = {"fundamental": ("fundamental_ransac", dict(threshold=2.0, refit=1)), "homography": ("homography_ransac", dict(threshold=2.0, refit=1)),
             "essential": ("essential_ransac", dict(threshold=2.0)), "similarity": ("similarity_ransac", dict(threshold=0.05, refit=1))}


def _pair(kind):
    method, options = PAIR_CALL[kind]

    @entry(method, (), ("sfmba_" + method,), masked=method + "_masked")
    def plain(be, I):
        p = I[kind]
        extra = (p["K"],) if "K" in p else ()
        return outputs_of(getattr(be, method)(p["a"], p["b"], *extra, p["ptr"], max_iters=p["H"], seed=5, **options))

    @entry(method + "_masked", (), ("sfmba_" + method,))
    def masked(be, I):
        p = I[kind]
        extra = (p["K"],) if "K" in p else ()
        return outputs_of(getattr(be, method)(p["a"], p["b"], *extra, p["ptr"], pair_use=p["use"], samples=p["samples"],
                                              want_hyp=True, **options))


for _kind in ("similarity", "fundamental", "homography", "essential"):
    _pair(_kind)


@entry("recover_pose", (), ("sfmba_recover_pose",), masked="recover_pose_masked")
def _(be, I):
    p = I["pose"]
    return outputs_of(be.recover_pose(p["E"], p["a"], p["b"], p["K"], p["ptr"]))


@entry("recover_pose_masked", (), ("sfmba_recover_pose",))
def _(be, I):
    p = I["pose"]
    return outputs_of(be.recover_pose(p["E"], p["a"], p["b"], p["K"], p["ptr"], pair_use=p["use"], min_depth=0.5))


@entry("match_descriptors", ("descriptors",), ("sfmba_set_descriptors", "sfmba_match_descriptors"), masked="match_descriptors_edges")
def _(be, I):
    out = dict(form=np.asarray(be.set_descriptors(I["descs"])))
    out.update(outputs_of(be.match_descriptors(ratio=0.9)))
    return out


@entry("match_descriptors_edges", ("descriptors",), ("sfmba_set_descriptors", "sfmba_match_descriptors"))
def _(be, I):
    out = dict(form=np.asarray(be.set_descriptors(I["descs"])))
    out.update(outputs_of(be.match_descriptors(I["match_edges"], ratio=0.9)))
    return out


@entry("build_tracks", ("tracks",), ("sfmba_build_tracks", "sfmba_get_tracks"), masked="build_tracks_masked")
def _(be, I):
    return outputs_of(be.build_tracks(*I["trk"]["batch"], conflicts=1))


@entry("build_tracks_masked", ("tracks",), ("sfmba_build_tracks", "sfmba_get_tracks"))
def _(be, I):
    return outputs_of(be.build_tracks(*I["trk"]["batch"], pair_use=I["trk"]["use"], min_length=3, max_length=12, conflicts=1))


def plan_masks(I, n_images, n_tracks):
    return mask(I["seed"] + 63, n_images, 0.6), mask(I["seed"] + 64, n_tracks, 0.5)


@entry("plan_views", ("tracks",), ("sfmba_build_tracks", "sfmba_get_tracks", "sfmba_plan_views"))
def _(be, I):
    t = be.build_tracks(*I["trk"]["batch"], conflicts=1)
    return outputs_of(be.plan_views(*plan_masks(I, len(t.img_ptr) - 1, t.n_tracks)))


@entry("assemble_problem", ("tracks",), ("sfmba_build_tracks", "sfmba_get_tracks", "sfmba_set_keypoints", "sfmba_assemble_problem",
                                        "sfmba_get_assembled"))
def _(be, I):
    t = be.build_tracks(*I["trk"]["batch"], conflicts=1)
    be.set_keypoints(I["trk"]["kp"])
    cam, trk = plan_masks(I, len(t.img_ptr) - 1, t.n_tracks)
    return outputs_of(be.assemble_problem(cam | mask(I["seed"] + 65, len(cam), 0.5), trk | mask(I["seed"] + 66, len(trk), 0.5), min_views=2))


MASKED = sorted({e["masked"] for e in ENTRIES.values()})        # one call per stage with every mask and optional output

# The functions of the binding that launch work and that no entry reaches, each with its reason.
NOT_IN_CATALOGUE = {
    "sfmba_set_exchange": "transport: sharded handles are out of scope, set_problem drops them",
    "sfmba_comm_get_unique_id": "multi-rank", "sfmba_comm_init": "multi-rank", "sfmba_comm_destroy": "multi-rank",
    "sfmba_p2p_export": "multi-rank", "sfmba_p2p_attach": "multi-rank", "sfmba_p2p_detach": "multi-rank",
    "sfmba_solve": "the in-out form of sfmba_solve_from, one code path (tests/test_gpu_boundary.py holds them equal)",
    "sfmba_time_kernel": "returns a time only",
    "sfmba_step_products": "test entry over one iteration's state, held entry by entry by tests/test_gpu_step_products.py",
    "sfmba_dense_schur": "test entry of the dense path, held by tests/test_gpu_entries.py",
    "sfmba_tr2d_solve": "host arithmetic, no handle state",
}
# ... and those that launch nothing: life cycle, options, getters
NO_WORK = ("sfmba_create", "sfmba_destroy", "sfmba_last_error", "sfmba_set_print", "sfmba_set_stream", "sfmba_set_precision",
           "sfmba_set_fixed_cameras", "sfmba_exchange_doubles", "sfmba_problem_reuse", "sfmba_p2p_calls", "sfmba_get_counters",
           "sfmba_get_form", "sfmba_get_mixed_operands", "sfmba_get_iteration_state", "sfmba_debug_option")


# ---- the pasts -----------------------------------------------------------------------------------------------------------------
def run_all(be, scale, names=None):
    """Every masked call of the catalogue (or `names`) once, on the inputs of `scale`."""
    I = inputs(scale)
    for name in (MASKED if names is None else names):
        ENTRIES[name]["fn"](be, I)


def past_larger(be, name):
    run_all(be, "larger")


def past_twin(be, name):
    """... and last of all the twin of the stage under test itself: the predecessor whose sizes every cache key matches."""
    run_all(be, "twin")
    run_all(be, "twin", [ENTRIES[name]["masked"]])


def past_smaller(be, name):
    run_all(be, "smaller")


def past_fp32(be, name):
    be.set_precision(32)
    # (covariance refuses fp32 storage: a refused call is part of this past)
    for n in MASKED:
        try:
            ENTRIES[n]["fn"](be, inputs("larger"))
        except ValueError:
            assert n.startswith("covariance"), n
    be.set_precision(64)


def refused(fn):
    """Run a call that the library or its wrapper is expected to refuse -> whether it did."""
    try:
        fn()
    except ValueError:
        return True
    return False


def failing_triangulations(I):
    """Keyword sets that drive `triangulate` on the tracks problem into every failing status (tests/test_host_history.py
    holds that by the restatement), and an x whose first camera is NaN (AT_INFINITY)."""
    x_nan = I["tracks"]["x"].copy()
    x_nan[:6] = np.nan
    return [(I["tracks"]["x"], kw) for kw in (dict(min_views=LONG + 2), dict(min_depth=1e3), dict(min_angle_deg=170.0),
                                               dict(max_error_px=1e-9))] + [(x_nan, {})]


def failing_resections(I):
    """Likewise for `resect` on the slices problem: FEW_VIEWS, BEHIND, HIGH_ERROR, and DEGENERATE from points that all coincide."""
    c = I["slices"]
    x_flat = c["x"].copy()
    x_flat[6 * c["args"][0]:] = 1.0
    return [(c["x"], kw) for kw in (dict(min_views=100), dict(min_depth=1e3), dict(max_rms_px=1e-9))] + [(x_flat, {})]


def past_failed(be, name):
    """Calls that end badly, then nothing else."""
    from sfmba import _capi
    I = inputs("entry")
    lib, h = be._lib, be._h
    # before any build on this handle
    assert lib.sfmba_get_tracks(h, None, None, None) == -1
    cam, trk = np.ones(2, dtype=np.uint8), np.ones(2, dtype=np.uint8)
    assert lib.sfmba_plan_views(h, 2, _capi.ptr(cam), 2, _capi.ptr(trk), None, None, None, None, None, None, None) == -1
    assert lib.sfmba_assemble_problem(h, 2, _capi.ptr(cam), 2, _capi.ptr(trk), None, None, None) == -1
    # an index out of range late in the arrays, then the valid call
    for key in ("ba", "tracks"):
        args = I[key].args if key == "ba" else I[key]["args"]
        bad = np.array(args[2], dtype=np.int64)
        bad[-3] = args[0]
        assert refused(lambda: be.set_problem(args[0], args[1], bad, args[3], args[4], args[5]))
        be.set_problem(*args)
    # covariance: no gauge (NaN matrices), an undetermined point
    for case, status in (("c11_nogauge", 1), ("c3_undropped", 2)):
        c = covariance_ref.case(case)
        be.set_problem(*c["args"])
        assert be.covariance(c["x"], gauge="auto" if c["gauge"] else "none", want_full=True).status == status
    # triangulation and resection into every failing status
    t, c = I["tracks"], I["slices"]
    be.set_problem(*t["args"])
    for x, kw in failing_triangulations(I):
        be.triangulate(x, **kw)
        be.triangulate_ransac(x, want_hyp=True, max_pairs=t["H"], **kw)
    be.set_problem(*c["args"])
    for x, kw in failing_resections(I):
        be.resect(x, **kw)
        be.resect_ransac(x, want_hyp=True, max_iters=c["H"], **kw)
    # one argument per stage that the C entry itself refuses (-1): the wrapper lets each of them through
    for what, call in refused_calls(be, I):
        assert refused(call), f"{what} was not refused"
    assert lib.sfmba_residuals(h, None, None) == -1
    assert lib.sfmba_build_tracks(h, 1, None, 0, None, None, None, None, None, None, None, None) == -1


def refused_calls(be, I):
    """(stage, call) pairs, each with one argument the library refuses: a NaN option, a sample position outside its
    set, form A asked of descriptors that are no integers.  The slices problem must be set."""
    nan = float("nan")
    c, f, g, e, s, p = (I[k] for k in ("slices", "fundamental", "homography", "essential", "similarity", "pose"))
    far = s["samples"].copy()
    far[0, 0, 0] = len(s["a"])

    def match_form_a_of_floats():
        be.set_descriptors([d.astype(np.float32) + 0.5 for d in I["descs"]])
        be.match_descriptors(form=1)

    return [
        ("reprojection_stats", lambda: be.reprojection_stats(c["x"], max_error_px=nan)),
        ("triangulate", lambda: be.triangulate(c["x"], xtol=nan)),
        ("triangulate_ransac", lambda: be.triangulate_ransac(c["x"], threshold=nan)),
        ("resect", lambda: be.resect(c["x"], xtol=nan)),
        ("resect_ransac", lambda: be.resect_ransac(c["x"], threshold=nan)),
        ("covariance", lambda: be.covariance(c["x"], rank_tol=nan)),
        ("fundamental_ransac", lambda: be.fundamental_ransac(f["a"], f["b"], f["ptr"], threshold=nan)),
        ("homography_ransac", lambda: be.homography_ransac(g["a"], g["b"], g["ptr"], threshold=nan)),
        ("essential_ransac", lambda: be.essential_ransac(e["a"], e["b"], e["K"], e["ptr"], threshold=nan)),
        ("similarity_ransac", lambda: be.similarity_ransac(s["a"], s["b"], s["ptr"], pair_use=s["use"], samples=far, threshold=0.05)),
        ("recover_pose", lambda: be.recover_pose(p["E"], p["a"], p["b"], p["K"], p["ptr"], min_depth=nan)),
        ("match_descriptors", match_form_a_of_floats),
    ]


# The stages that share buffers: the members of a family run immediately before the call under test, masked, on the twin's
# content, in the order given ("family") and reversed ("family_reversed").
FAMILIES = (
    ("triangulate", "triangulate_masked", "triangulate_ransac", "triangulate_ransac_masked"),
    ("resect_ransac", "resect_ransac_masked", "resect", "resect_masked"),
    ("similarity_ransac", "similarity_ransac_masked", "fundamental_ransac", "fundamental_ransac_masked", "homography_ransac",
     "homography_ransac_masked", "essential_ransac", "essential_ransac_masked", "recover_pose", "recover_pose_masked"),
    ("covariance_marginal", "covariance_conditional", "reprojection_stats", "reprojection_stats_filtered", "resect", "resect_masked"),
)


def siblings(name):
    """The masked calls of the other stages of every family `name` belongs to, in family order."""
    out = []
    for fam in FAMILIES:
        if name in fam:
            own = ENTRIES[name]["masked"]
            out += [m for m in dict.fromkeys(ENTRIES[n]["masked"] for n in fam) if m != own and m not in out]
    return out


def past_family(be, name):
    run_all(be, "twin", siblings(name))


def past_family_reversed(be, name):
    run_all(be, "twin", siblings(name)[::-1])


PASTS = {"larger": past_larger, "twin": past_twin, "smaller": past_smaller, "failed": past_failed, "fp32": past_fp32,
         "family": past_family, "family_reversed": past_family_reversed}

NO_FAMILY = "shares no buffer with a sibling stage: it has no family"
ONE_SIBLING = "its family has one other stage: the reversed order is the same past"
EXCLUDED = {}
for _name in ENTRIES:
    if not siblings(_name):
        EXCLUDED[(_name, "family")] = EXCLUDED[(_name, "family_reversed")] = NO_FAMILY
    elif len(siblings(_name)) == 1:
        EXCLUDED[(_name, "family_reversed")] = ONE_SIBLING
PAIRS = [(e, p) for e in ENTRIES for p in PASTS if (e, p) not in EXCLUDED]


# ---- problem sequences for the solver entries ------------------------------------------------------------------------------------
def start_vector(C, P, seed=0):
    """Cameras near the origin looking down +z, points ten units in front: finite residuals for any pixels."""
    rng = np.random.default_rng(seed)
    cams = np.hstack([rng.normal(0.0, 0.1, (C, 3)), rng.normal(0.0, 0.5, (C, 3))])
    pts = rng.normal(0.0, 1.0, (P, 3)) + [0.0, 0.0, 10.0]
    return np.concatenate([cams.ravel(), pts.ravel()])


def vectors(C, P, seed=1):
    rng = np.random.default_rng(seed)
    return dict(dc=rng.uniform(1.0, 20.0, 6 * C), dp=rng.uniform(1.0, 20.0, 3 * P), v=rng.normal(size=6 * C))


def step(C, P, cam, pt, uv, K=K_PIX, fixed=(), f32=0, packed=0, x0=None, **more):
    """One set_problem of a sequence.  more: ok (False: the call is refused), reuse (what problem_reuse()[0] must be,
    None: not fixed), consumers (also run covariance, statistics and resection after it), note."""
    s = dict(C=int(C), P=int(P), cam=np.asarray(cam, np.int64), pt=np.asarray(pt, np.int64), uv=np.asarray(uv), K=np.asarray(K, np.float64),
             fixed=tuple(fixed), f32=int(f32), packed=int(packed), x0=start_vector(C, P) if x0 is None else x0, ok=True, reuse=None,
             consumers=False, note="")
    s.update(more)
    return s


def from_host_case(name):
    """A sequence of tests/test_host_tables.py's `case()` as steps, with the re-use its `expected()` defines."""
    import test_host_tables as tht
    calls, exp = tht.case(name), tht.expected_of(name)
    return [step(c["C"], c["P"], c["cam"], c["pt"], c["uv"], fixed=c["fixed"], f32=c["f32"], packed=c["plan"]["packed_upload"],
                 ok=bool(e["ok"]), reuse=e.get("fdiff"), note=f"{name}[{k}]") for k, (c, e) in enumerate(zip(calls, exp))]


def as_host_calls(steps):
    """Steps in the form `test_host_tables.expected()` takes."""
    import test_host_tables as tht
    return [tht.call(s["C"], s["P"], s["cam"], s["pt"], s["uv"], fixed=s["fixed"], f32=s["f32"], packed_upload=s["packed"]) for s in steps]


@functools.lru_cache(maxsize=None)
def sequence(name):
    if name in ("reuse", "reuse_packed", "bad_index"):
        steps = from_host_case(name)
        if name == "reuse":                                    # ... and back to fp64 (the host case ends in fp32)
            last = steps[-1]
            steps.append(dict(last, f32=0, reuse=0, note="reuse[fp64 again]"))
        return steps
    pb = inputs("entry")["ba"]
    C, P, cam, pt, uv, K = pb.args
    if name == "unsorted":                                     # unsorted -> its sorted prefix -> unsorted: nothing to re-use in between
        sh = np.random.default_rng(8).permutation(len(pt))
        n = len(pt) - 300
        return [step(C, P, cam[sh], pt[sh], uv[sh], K, x0=pb.x0, reuse=0, note="unsorted"),
                step(C, P, cam[:n], pt[:n], uv[:n], K, x0=pb.x0, reuse=0, note="sorted prefix"),
                step(C, P, cam[sh], pt[sh], uv[sh], K, x0=pb.x0, reuse=0, note="unsorted again")]
    if name == "same_arrays":                                  # problem_gen stays: everything derived from it must still be right
        N = len(pt)
        K2 = K.copy()
        K2[0, 0], K2[1, 1], K2[0, 2] = 2800.0, 2850.0, 1400.0
        x_more = np.concatenate([pb.x0[:6 * C], start_vector(3, 0, seed=5), pb.x0[6 * C:]])
        mk = lambda **kw: step(kw.pop("C", C), P, cam, pt, uv, kw.pop("K", K), x0=kw.pop("x0", pb.x0), **kw)
        return [mk(reuse=0, note="first"), mk(K=K2, reuse=N, note="another K"), mk(reuse=N, note="K back")] + \
               [mk(fixed=f, reuse=N, consumers=True, note=f"held {f}") for f in ((), (0,), (0, 3), ())] + \
               [mk(C=C + 3, x0=x_more, reuse=N, consumers=True, note="three cameras nobody observes"), mk(reuse=N, consumers=True, note="back")]
    raise KeyError(name)


SEQUENCES = ("reuse", "reuse_packed", "bad_index", "unsorted", "same_arrays")


def apply_step(be, s):
    """The step's set_problem on a handle -> whether it was accepted."""
    be.debug_option("packed_upload", s["packed"])
    be.set_precision(32 if s["f32"] else 64)
    be.set_fixed_cameras(s["fixed"])
    return not refused(lambda: be.set_problem(s["C"], s["P"], s["cam"], s["pt"], s["uv"], s["K"]))


def step_outputs(be, s):
    """Every solver entry on the step's problem, and the consumers that read the cached permutation where the step asks."""
    out = solver_outputs(be, s["x0"], vectors(s["C"], s["P"]), max_nfev=6)
    if s["consumers"]:
        out["covariance_conditional"] = outputs_of(be.covariance(s["x0"], kind="conditional"))
        out["reprojection_stats"] = outputs_of(be.reprojection_stats(s["x0"]))
        out["resect"] = outputs_of(be.resect(s["x0"], start=1))
    return out
