"""Bit identity of the consumers (reprojection statistics, triangulation, resection, and the two-view calls -- F, homography,
essential, pose -- the robust resection and the covariance call where both builds have them) between two builds of the library.  Usage: python tools/ab_consumer_bits.py LIB_A LIB_B [--out DIR]

One fresh child process per library (SFMBA_LIB), each under its own time limit; the tool stops at the first child that
does not exit cleanly.  A child runs the three calls over inputs that reach every form of the kernels -- the long-run,
ring and boundary problems of the tests, 1200 cameras (the camera table does not fit the LDS), camera slices at the edges
of k_resect's strided loop -- in 64- and 32-bit storage, with and without select / obs_use, start 0 and 1, max_iter 0 and
default, and writes every returned array to DIR/consumer_bits_<a|b>.npz (DIR: a fresh temporary folder unless --out names
one).  The parent compares the two files byte for byte."""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "sfm-python_amd"), os.path.join(ROOT, "tests")]
import numpy as np

CHILD_SECONDS = 240


def inputs():
    import consumer_inputs as ci
    import sfmba
    from kernel_source import kernel_constant
    L = kernel_constant("kStatsLongTrack")
    yield "long_runs", ci.long_run_problem()
    yield "ring", ci.ring_tracks(40, 705, {5: 2, 70: L - 1, 71: L, 300: L + 1, 640: 40}, cam_seed=9, seed=17)
    yield "boundary", ci.boundary_problem()
    pb = sfmba.make_problem(1200, 800, 6000, seed=6)
    yield "many_cameras", (pb.x0, pb.args)
    yield "camera_slices", ci.camera_slices_problem([1, 255, 256, 257, 1024, 1025])


def kernel_constant_of(name):
    from kernel_source import kernel_constant
    return kernel_constant(name)


def child(out_path):
    import sfmba
    from sfmba.backend import ReprojectionStats
    be = sfmba.Backend(0)
    out = {}
    for name, (x, args) in inputs():
        C, P, ci, pi, uv, K = args
        rng = np.random.default_rng(5)
        masks = (rng.random(len(ci)) < 0.85, rng.random(P) < 0.7, rng.random(C) < 0.7)
        for bits in (64, 32):
            be.set_precision(bits)
            be.set_problem(*args)
            for tag, kw in (("default", {}), ("filter", dict(max_error_px=1.0, min_depth=0.0, min_angle_deg=1.0, min_views=2))):
                st = be.reprojection_stats(x, **kw)
                for f in ReprojectionStats._ARRAYS:
                    out[f"{name}/{bits}/stats/{tag}/{f}"] = getattr(st, f)
                out[f"{name}/{bits}/stats/{tag}/summary"] = np.array([getattr(st, f) for f in ReprojectionStats._SUMMARY], dtype=np.float64)
            for m, (use, psel, csel) in (("all", (None, None, None)), ("masked", masks)):
                for it in ({"max_iter": 0}, {}):
                    t = be.triangulate(x, select=psel, obs_use=use, **it)
                    key = f"{name}/{bits}/tri/{m}/{'linear' if it else 'refined'}"
                    for f in ("points", "status", "views", "iters", "rms_err", "angle_deg"):
                        out[f"{key}/{f}"] = getattr(t, f)
                    out[f"{key}/n_ok"] = np.array([t.n_ok])
                    for start in (0, 1):
                        r = be.resect(x, select=csel, obs_use=use, start=start, **it)
                        key = f"{name}/{bits}/resect/{m}/start{start}/{'linear' if it else 'refined'}"
                        for f in ("cameras", "status", "views", "iters", "rms_err"):
                            out[f"{key}/{f}"] = getattr(r, f)
                        out[f"{key}/n_ok"] = np.array([r.n_ok])
                if hasattr(be._lib, "sfmba_resect_ransac"):  # (an older build has it not) drawn samples, refined and not
                    for refine in (0, 1):
                        r = be.resect_ransac(x, select=csel, obs_use=use, want_hyp=True, max_iters=96, threshold=2.0, seed=4,
                                             min_views=4, refine=refine)
                        for f in ("cameras", "hyp", "inlier_mask", "status", "views", "inliers", "best", "best_sol", "success",
                                  "iters", "rms_err", "hyp_inliers"):
                            out[f"pnp/{name}/{bits}/{m}/refine{refine}/{f}"] = getattr(r, f)
    # the two-view calls: a batch that reaches the staged and the unstaged form, every status, a mask, drawn and given samples
    if hasattr(be._lib, "sfmba_fundamental_ransac"):      # (an older build has neither)
        import two_view_ref as tv
        L = kernel_constant_of("kTwoViewLdsPairs")
        rng = np.random.default_rng(6)
        K = sfmba.K_SCEAUX
        made = [tv.make_pairs(rng, n, K, noise=0.3, outliers=0.25) for n in (7, 8, 65, 1900, L + 1)]
        ptr = np.concatenate([[0], np.cumsum([len(m[0]) for m in made])]).astype(np.int64)
        p1, p2 = np.concatenate([m[0] for m in made]), np.concatenate([m[1] for m in made])
        use = rng.random(len(p1)) < 0.9
        smp = np.stack([tv.draw_samples(3, e, 40, 8) for e in range(len(made))])
        for tag, kw in (("drawn", dict(max_iters=40, seed=3)), ("masked", dict(max_iters=40, seed=3, pair_use=use)), ("given", dict(samples=smp))):
            est = be.fundamental_ransac(p1, p2, edge_ptr=ptr, threshold=1.0, refit=1, want_hyp=True, **kw)
            for f in ("F", "F_refit", "inlier_mask", "inliers", "best", "success", "status", "hyp_inliers"):
                out[f"two_view/64/ransac/{tag}/{f}"] = getattr(est, f)
        if hasattr(be._lib, "sfmba_homography_ransac"):   # the same batch and options through the homography model
            import homography_ref as hr
            smp4 = np.stack([hr.draw_samples4(3, e, 40, int(ptr[e + 1] - ptr[e])) for e in range(len(made))])
            for tag, kw in (("drawn", dict(max_iters=40, seed=3)), ("masked", dict(max_iters=40, seed=3, pair_use=use)), ("given", dict(samples=smp4))):
                est = be.homography_ransac(p1, p2, edge_ptr=ptr, threshold=1.0, refit=1, want_hyp=True, **kw)
                for f in ("H", "H_refit", "inlier_mask", "refit_mask", "inliers", "refit_inliers", "best", "success", "status", "hyp_inliers"):
                    out[f"two_view/64/homography/{tag}/{f}"] = getattr(est, f)
        if hasattr(be._lib, "sfmba_essential_ransac"):    # the same batch behind an edge of 4 pairs (FEW_PAIRS for five-pair samples)
            import essential_ref as er
            few = tv.make_pairs(rng, 4, K, noise=0.3)
            eptr = np.concatenate([[0], 4 + ptr]).astype(np.int64)
            e1, e2, euse = np.concatenate([few[0], p1]), np.concatenate([few[1], p2]), np.concatenate([np.ones(4, dtype=bool), use])
            sizes = np.diff(eptr)
            smp5 = np.stack([er.draw_samples5(3, e, 40, int(n)) if n >= 5 else np.zeros((40, 5), dtype=np.int32) for e, n in enumerate(sizes)])
            for tag, kw in (("drawn", dict(max_iters=40, seed=3)), ("masked", dict(max_iters=40, seed=3, pair_use=euse)), ("given", dict(samples=smp5))):
                est = be.essential_ransac(e1, e2, K, edge_ptr=eptr, threshold=1.0, want_hyp=True, **kw)
                for f in ("E", "inlier_mask", "inliers", "best", "best_root", "success", "status", "hyp_inliers", "hyp_roots"):
                    out[f"two_view/64/essential/{tag}/{f}"] = getattr(est, f)
        Es = np.stack([tv.essential_from_pose(m[2], m[3]) for m in made])
        Es[1] = 0.0
        for tag, kw in (("all", {}), ("masked", dict(pair_use=use)), ("deep", dict(min_depth=6.0))):
            pose = be.recover_pose(Es, p1, p2, K, edge_ptr=ptr, **kw)
            for f in ("R", "t", "front_mask", "X", "angle_deg", "front", "front_all", "sum_err", "status"):
                out[f"two_view/64/pose/{tag}/{f}"] = getattr(pose, f)
    # the covariance call: marginal at 11 and 21 cameras (lane and wave form of the point sweep), conditional at 40
    if hasattr(be._lib, "sfmba_covariance"):              # (an older build has it not)
        import covariance_ref as cr
        for name in ("c11_dup", "c21", "grid21", "cond40"):
            c = cr.case(name)
            be.set_precision(64)
            be.set_fixed_cameras(c["fixed"])
            be.set_problem(*c["args"])
            for kind in (("conditional",) if c["kind"] else ("marginal", "conditional")):
                cov = be.covariance(c["x"], kind=kind, want_full=True)
                for f in ("cam_cov", "cam_full", "cam_sigma", "pt_cov", "pt_sigma", "pt_status", "held"):
                    out[f"cov/{name}/{kind}/{f}"] = getattr(cov, f)
                out[f"cov/{name}/{kind}/info"] = np.array([cov.sigma2, cov.cost, cov.min_pivot_rel, cov.dof, cov.status], dtype=np.float64)
    be.close()
    np.savez(out_path, **{k.replace("/", "|"): v for k, v in out.items()})


def main():
    argv = sys.argv[1:]
    if argv[:1] == ["--child"]:
        return child(argv[1])
    out_dir = None
    if "--out" in argv:
        k = argv.index("--out")
        out_dir = argv[k + 1]
        del argv[k:k + 2]
    lib_a, lib_b = (os.path.abspath(p) for p in argv)
    if out_dir is None:
        out_dir = tempfile.mkdtemp(prefix="consumer_bits_")
    os.makedirs(out_dir, exist_ok=True)
    files = []
    for tag, lib in (("a", lib_a), ("b", lib_b)):
        path = os.path.join(out_dir, f"consumer_bits_{tag}.npz")
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path], env=dict(os.environ, SFMBA_LIB=lib),
                                timeout=CHILD_SECONDS).returncode
        except subprocess.TimeoutExpired:
            rc = "time limit"
        if rc != 0:
            print(f"{lib}: the child ended with {rc}; stopping")
            return 2
        files.append(np.load(path))
    a, b = files
    class Without:
        def __init__(self, f, prefix):
            self.f, self.files = f, [k for k in f.files if not k.startswith(prefix)]

        def __getitem__(self, k):
            return self.f[k]

    for prefix, what in (("two_view|", "the two-view calls"), ("pnp|", "the robust resection"), ("cov|", "the covariance call")):
        only = [f for f in (a, b) if any(k.startswith(prefix) for k in f.files)]
        if len(only) == 1:                                       # one build has not got the call: nothing to compare it with
            print(f"  (only one build has {what}: its arrays are left out)")
            a, b = Without(a, prefix), Without(b, prefix)
    print(f"A = {lib_a}\nB = {lib_b}")
    differ = [k for k in a.files if k not in b.files or a[k].dtype != b[k].dtype or a[k].tobytes() != b[k].tobytes()]
    differ += [k for k in b.files if k not in a.files]
    groups = {}
    for k in a.files:
        g = "/".join(k.split("|")[:3])
        n, bad = groups.get(g, (0, 0))
        groups[g] = (n + 1, bad + (k in differ))
    for g, (n, bad) in groups.items():
        print(f"  {g:32s} {n:4d} arrays  {'identical' if not bad else '%d DIFFER' % bad}")
    nbytes = sum(a[k].nbytes for k in a.files)
    print(f"{len(a.files)} arrays, {nbytes} bytes: " + ("every array identical" if not differ else f"{len(differ)} arrays differ"))
    for k in differ[:20]:
        print("  differs:", k.replace("|", "/"))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
