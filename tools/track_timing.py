"""Timing of track building: sfmba_build_tracks from its own `kernel_us` (profile = 1: HIP events
round all launches of a call) and the whole `Backend.build_tracks` call (argument checks, upload, kernels, download) on
synthetic match graphs at the project's scales, 1000 images / ~1M observations and 5000 images / ~10M observations, beside
`scipy.sparse.csgraph.connected_components` plus the numpy grouping that yields the same CSR on the same box.

The graphs: track lengths are drawn as `make_problem` draws the observations of a point (every point once, the rest
uniformly), every observation in a random image, repeats of (point, image) dropped; the features of an image are its
observations in a random order, and every track is chained through its images in ascending order, one pair per link,
the pairs grouped into edges (u > v).  Every figure is the median of ROUNDS warm calls; min and max are the scatter.  No
speed threshold is attached: the CPU figure beside it is the yardstick.

Each step runs in a child process of its own under a time limit; the first step that fails ends the run.
Usage: python tools/track_timing.py [--out profiles/track_timing.txt]"""
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
STEP_SECONDS = 240
STEPS = tuple(f"{impl}-{scale}" for scale in SCALES for impl in ("sfmba", "scipy"))


def match_graph(scale):
    C, P, n_obs = SCALES[scale]
    rng = np.random.default_rng(7)
    pt = np.concatenate([np.arange(P, dtype=np.int64), rng.integers(0, P, n_obs - P, dtype=np.int64)])
    cam = rng.integers(0, C, n_obs, dtype=np.int64)
    key = np.unique(pt * C + cam)                                # sorted by (point, image), repeats dropped
    pt, cam = key // C, key % C
    # rows: the observations of an image in a random order
    shuffle = rng.permutation(len(key))
    by_image = shuffle[np.argsort(cam[shuffle], kind="stable")]
    img_ptr = np.concatenate([[0], np.cumsum(np.bincount(cam, minlength=C))]).astype(np.int64)
    row = np.empty(len(key), dtype=np.int64)
    row[by_image] = np.arange(len(key)) - img_ptr[cam[by_image]]
    link = np.flatnonzero(pt[1:] == pt[:-1])                     # observation k + 1 is the same point in a later image
    u, v = cam[link + 1], cam[link]
    order = np.argsort(u * C + v, kind="stable")
    ekey, first = np.unique((u * C + v)[order], return_index=True)
    edges = np.stack([ekey // C, ekey % C], axis=1).astype(np.int32)
    pair_ptr = np.concatenate([first, [len(link)]]).astype(np.int64)
    pairs = np.stack([row[link + 1], row[link]], axis=1)[order].astype(np.int32)
    truth = dict(tracks=int((np.bincount(pt, minlength=P) >= 2).sum()), observations=int(len(key)))
    return (img_ptr, edges, pair_ptr, pairs), truth


def step_sfmba(scale):
    import sfmba
    batch, truth = match_graph(scale)
    be = sfmba.Backend(0)
    t = be.build_tracks(*batch, profile=1)                        # warm-up: code objects
    us, call = [], []
    for _ in range(ROUNDS):
        t0 = time.perf_counter()
        t = be.build_tracks(*batch, profile=1)
        call.append(1e6 * (time.perf_counter() - t0))
        us.append(t.kernel_us)
    be.close()
    assert t.n_tracks == truth["tracks"] and t.counts["conflict"] == 0
    return dict(us=us, call=call, tracks=t.n_tracks, obs=t.counts["observations"], features=int(batch[0][-1]),
                pairs=int(len(batch[3])), edges=int(len(batch[1])), digest=int(t.track_feat.astype(np.int64).sum() % (1 << 61)))


def cpu_tracks(img_ptr, edges, pair_ptr, pairs):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    N = int(img_ptr[-1])
    g = np.repeat(img_ptr[edges], np.diff(pair_ptr), axis=0) + pairs
    _, lab = connected_components(coo_matrix((np.ones(len(g), dtype=np.int8), (g[:, 0], g[:, 1])), shape=(N, N)), directed=False)
    size = np.bincount(lab)
    feat = np.flatnonzero(size[lab] >= 2)                         # ascending ids; grouped by the label's first member
    smallest = np.full(len(size), N, dtype=np.int64)
    np.minimum.at(smallest, lab[feat], feat)
    order = np.argsort(smallest[lab[feat]], kind="stable")
    track_feat = feat[order]
    image = np.searchsorted(img_ptr, track_feat, side="right") - 1
    starts = np.flatnonzero(np.diff(smallest[lab[track_feat]], prepend=-1))
    clash = (image[1:] == image[:-1]) & (lab[track_feat][1:] == lab[track_feat][:-1])
    return np.append(starts, len(track_feat)), track_feat, image, int(clash.sum())


def step_scipy(scale):
    batch, truth = match_graph(scale)
    cpu_tracks(*batch)
    us = []
    for _ in range(ROUNDS):
        t0 = time.perf_counter()
        ptr, feat, image, clashes = cpu_tracks(*batch)
        us.append(1e6 * (time.perf_counter() - t0))
    assert len(ptr) - 1 == truth["tracks"] and clashes == 0
    return dict(us=us, tracks=len(ptr) - 1, obs=int(len(feat)), digest=int(feat.astype(np.int64).sum() % (1 << 61)))


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--step":
        impl, scale = sys.argv[2].split("-")
        print("RESULT " + json.dumps((step_sfmba if impl == "sfmba" else step_scipy)(scale)), flush=True)
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
    lines = [f"track building, median of {ROUNDS} warm calls [min .. max], microseconds"]

    def row(label, v):
        v = np.array(v)
        return f"  {label:58s} {np.median(v):12.1f} [{v.min():12.1f} .. {v.max():12.1f}]"
    for scale in SCALES:
        g, c = results[f"sfmba-{scale}"], results[f"scipy-{scale}"]
        same = (g["tracks"], g["obs"], g["digest"]) == (c["tracks"], c["obs"], c["digest"])
        lines.append(f"{scale} images: {g['features']} features, {g['edges']} edges, {g['pairs']} pairs -> {g['tracks']} tracks, "
                     f"{g['obs']} observations" + ("" if same else "  -- THE TWO RESULTS DIFFER"))
        lines.append(row("sfmba_build_tracks, kernel_us (12 launches)", g["us"]))
        lines.append(row("Backend.build_tracks, whole call", g["call"]))
        lines.append(row("scipy connected_components + numpy grouping (CPU)", c["us"]))
        lines.append(f"  whole call: {np.median(c['us']) / np.median(g['call']):.2f} x the speed of the CPU yardstick; "
                     f"kernels alone: {np.median(c['us']) / np.median(g['us']):.1f} x")
    text = "\n".join(lines)
    print(text)
    if out_path:
        with open(out_path, "w") as f:
            f.write(text + "\n")


main()
