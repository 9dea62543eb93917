"""Timing of the plan stage: sfmba_plan_views and sfmba_assemble_problem + sfmba_get_assembled from
their own `kernel_us` (profile = 1: HIP events round the launches of a call) and as whole Python calls (argument checks,
mask upload, kernels, download), on the two track graphs of tools/track_timing.py -- 1000 images / ~1M observations and
5000 images / ~10M observations -- with half the images registered and half the tracks known, beside a vectorised numpy
version of the same (np.bincount / boolean indexing over the CSR) on the same box: the yardstick.  Then sfmba.reconstruct
on a 50-camera ring, its time per round split by stage.

Every figure of the first part is the median of ROUNDS warm calls; min and max are the scatter.  No speed threshold is
attached.  Each step runs in a child process of its own under a time limit; the first step that fails ends the run.
Usage: python tools/plan_timing.py [--out profiles/plan_timing.txt]"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "sfm-python_amd"), os.path.join(ROOT, "tests")]
import numpy as np

SCALES = {"1000": (1000, 100000, 1000000), "5000": (5000, 1000000, 10000000)}     # images, points, observations drawn
ROUNDS = 5
STEP_SECONDS = 300
STEPS = tuple(f"plan-{scale}" for scale in SCALES) + ("reconstruct-50",)
RING = dict(n_cameras=50, n_points=2000, n_obs=30000, seed=3)


def match_graph(scale):
    """The graph of tools/track_timing.py (the same draws from the same seed)."""
    C, P, n_obs = SCALES[scale]
    rng = np.random.default_rng(7)
    pt = np.concatenate([np.arange(P, dtype=np.int64), rng.integers(0, P, n_obs - P, dtype=np.int64)])
    cam = rng.integers(0, C, n_obs, dtype=np.int64)
    key = np.unique(pt * C + cam)
    pt, cam = key // C, key % C
    shuffle = rng.permutation(len(key))
    by_image = shuffle[np.argsort(cam[shuffle], kind="stable")]
    img_ptr = np.concatenate([[0], np.cumsum(np.bincount(cam, minlength=C))]).astype(np.int64)
    row = np.empty(len(key), dtype=np.int64)
    row[by_image] = np.arange(len(key)) - img_ptr[cam[by_image]]
    link = np.flatnonzero(pt[1:] == pt[:-1])
    u, v = cam[link + 1], cam[link]
    order = np.argsort(u * C + v, kind="stable")
    ekey, first = np.unique((u * C + v)[order], return_index=True)
    edges = np.stack([ekey // C, ekey % C], axis=1).astype(np.int32)
    pair_ptr = np.concatenate([first, [len(link)]]).astype(np.int64)
    pairs = np.stack([row[link + 1], row[link]], axis=1)[order].astype(np.int32)
    return img_ptr, edges, pair_ptr, pairs


def numpy_plan_views(t, point_of_obs, image_of_feat, cam_reg, trk_known):
    views = np.bincount(point_of_obs[cam_reg[t.track_image]], minlength=t.n_tracks).astype(np.int32)
    in_track = t.feat_track >= 0
    ft = t.feat_track[in_track]
    img = image_of_feat[in_track]
    n = len(t.img_ptr) - 1
    known = trk_known[ft]
    gain = ~known & (views[ft] - cam_reg[img] >= 1)
    return (views, np.bincount(img, minlength=n).astype(np.int32), np.bincount(img[known], minlength=n).astype(np.int32),
            np.bincount(img[gain], minlength=n).astype(np.int32))


def numpy_assemble(t, point_of_obs, allpts, cam_use, trk_use, min_views=2):
    used = trk_use[point_of_obs] & cam_use[t.track_image]
    kept = np.bincount(point_of_obs[used], minlength=t.n_tracks) >= min_views
    sel = used & kept[point_of_obs]
    pt_of = np.flatnonzero(kept).astype(np.int32)
    images = t.track_image[sel]
    present = np.bincount(images, minlength=len(t.img_ptr) - 1) > 0
    cam_of = np.flatnonzero(present).astype(np.int32)
    obs_feat = t.track_feat[sel]
    return (cam_of, pt_of, (np.cumsum(present) - 1)[images].astype(np.int64), (np.cumsum(kept) - 1)[point_of_obs[sel]].astype(np.int64),
            obs_feat, allpts[obs_feat])


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return 1e6 * (time.perf_counter() - t0), out


def step_plan(scale):
    import sfmba
    batch = match_graph(scale)
    rng = np.random.default_rng(11)
    be = sfmba.Backend(0)
    t = be.build_tracks(*batch)
    n_images = len(t.img_ptr) - 1
    pts = [rng.uniform(0.0, 4000.0, (int(n), 2)) for n in np.diff(t.img_ptr)]
    allpts = np.concatenate(pts)
    be.set_keypoints(pts)
    cam, trk = rng.random(n_images) < 0.5, rng.random(t.n_tracks) < 0.5
    point_of_obs = np.repeat(np.arange(t.n_tracks), np.diff(t.track_ptr))
    image_of_feat = np.repeat(np.arange(n_images), np.diff(t.img_ptr))
    every = np.ones(t.n_tracks, dtype=bool)
    be.plan_views(cam, trk, profile=1), be.assemble_problem(cam, every, profile=1)              # warm-up: code objects
    res = dict(views_us=[], views_call=[], views_numpy=[], sub_us=[], sub_call=[], sub_numpy=[])
    for _ in range(ROUNDS):
        us, v = timed(lambda: be.plan_views(cam, trk, profile=1))
        res["views_call"].append(us), res["views_us"].append(v.kernel_us)
        us, s = timed(lambda: be.assemble_problem(cam, every, profile=1))
        res["sub_call"].append(us), res["sub_us"].append(s.kernel_us)
        us, nv = timed(lambda: numpy_plan_views(t, point_of_obs, image_of_feat, cam, trk))
        res["views_numpy"].append(us)
        us, ns = timed(lambda: numpy_assemble(t, point_of_obs, allpts, cam, every))
        res["sub_numpy"].append(us)
    be.close()
    same = all(np.array_equal(a, b) for a, b in zip(nv, (v.trk_reg_views, v.img_tracks, v.img_known, v.img_gain)))
    same = same and all(np.array_equal(a, b) for a, b in zip(ns, (s.cam_of, s.pt_of, s.camera_indices, s.point_indices, s.obs_feat, s.points_2d)))
    res.update(same=bool(same), images=n_images, tracks=t.n_tracks, obs=t.counts["observations"], features=int(t.img_ptr[-1]),
               sub=[s.n_cameras, s.n_points, s.n_obs])
    return res


def step_reconstruct(_):
    import sfmba
    import test_gpu_reconstruct as T
    scene = T.Scene(params=RING)
    be = sfmba.Backend(0)
    spent = {}

    def wrap(name, label):
        inner = getattr(be, name)

        def outer(*a, **k):
            t0 = time.perf_counter()
            out = inner(*a, **k)
            spent[label] = spent.get(label, 0.0) + 1e3 * (time.perf_counter() - t0)
            return out
        setattr(be, name, outer)
    for name, label in (("plan_views", "plan + assemble"), ("assemble_problem", "plan + assemble"), ("set_problem", "set_problem"),
                        ("resect_ransac", "resection"), ("triangulate", "triangulation"), ("solve", "solve"),
                        ("reprojection_stats", "filter (statistics)")):
        wrap(name, label)
    sfmba.reconstruct(scene.matches, scene.pts, scene.K, init=(1, 0), batch=1, backend=be)      # warm-up: code objects
    spent.clear()
    t0 = time.perf_counter()
    rec = sfmba.reconstruct(scene.matches, scene.pts, scene.K, init=(1, 0), batch=1, backend=be)
    total = 1e3 * (time.perf_counter() - t0)
    be.close()
    return dict(spent=spent, total=total, rounds=len(rec.rounds), registered=int(rec.registered.sum()), known=int(rec.known.sum()),
                tracks=rec.tracks.n_tracks, obs=rec.tracks.counts["observations"])


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--step":
        kind, scale = sys.argv[2].split("-")
        print("RESULT " + json.dumps((step_plan if kind == "plan" else step_reconstruct)(scale)), flush=True)
        return
    out_path = sys.argv[2] if len(sys.argv) > 2 and sys.argv[1] == "--out" else None
    results = {}
    for name in STEPS:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name], capture_output=True, text=True,
                               timeout=STEP_SECONDS)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"step {name} ran into its time limit of {STEP_SECONDS} s; nothing more is started")
        line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            raise SystemExit(f"step {name} failed with exit status {p.returncode}; nothing more is started")
        results[name] = json.loads(line[-1][7:])
    lines = [f"plan stage, half the images registered, half the tracks known; median of {ROUNDS} warm calls [min .. max], microseconds"]

    def row(label, v):
        v = np.array(v)
        return f"  {label:66s} {np.median(v):12.1f} [{v.min():12.1f} .. {v.max():12.1f}]"
    for scale in SCALES:
        r = results[f"plan-{scale}"]
        lines.append(f"{r['images']} images, {r['features']} features, {r['tracks']} tracks, {r['obs']} observations; sub-problem "
                     f"{r['sub'][0]} cameras, {r['sub'][1]} points, {r['sub'][2]} observations" + ("" if r["same"] else "  -- THE TWO RESULTS DIFFER"))
        lines.append(row("sfmba_plan_views, kernel_us (2 launches)", r["views_us"]))
        lines.append(row("Backend.plan_views, whole call", r["views_call"]))
        lines.append(row("numpy bincount version (CPU)", r["views_numpy"]))
        lines.append(row("sfmba_assemble_problem, kernel_us (9 launches)", r["sub_us"]))
        lines.append(row("Backend.assemble_problem, whole call (with sfmba_get_assembled)", r["sub_call"]))
        lines.append(row("numpy boolean-indexing version (CPU)", r["sub_numpy"]))
        lines.append(f"  whole calls against numpy: plan_views {np.median(r['views_numpy']) / np.median(r['views_call']):.2f} x, "
                     f"assemble_problem {np.median(r['sub_numpy']) / np.median(r['sub_call']):.2f} x the speed of the yardstick")
    r = results["reconstruct-50"]
    lines.append(f"sfmba.reconstruct, ring of {RING['n_cameras']} cameras, {r['tracks']} tracks, {r['obs']} observations, batch=1: "
                 f"{r['registered']} images registered, {r['known']} tracks known, {r['rounds']} rounds, {r['total']:.1f} ms (second run)")
    other = r["total"] - sum(r["spent"].values())
    for label, ms in list(r["spent"].items()) + [("host (numpy, Python)", other)]:
        lines.append(f"  {label:28s} {ms / max(r['rounds'], 1):9.3f} ms per round   {100.0 * ms / r['total']:5.1f} %")
    text = "\n".join(lines)
    print(text)
    if out_path:
        with open(out_path, "w") as f:
            f.write(text + "\n")


main()
