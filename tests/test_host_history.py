"""The catalogue, the pasts and the sequences of tests/handle_history.py, checked without a device: that the catalogue
reaches the whole binding, that "twin", "larger" and "smaller" are what their names say, that the sequences' expected
re-use is the one tests/test_host_tables.py defines, and that the numpy restatements accept the catalogue's inputs."""
import numpy as np
import pytest

import covariance_ref
import essential_ref
import handle_history as hh
import homography_ref
import match_ref
import plan_ref
import pnp_ransac_ref
import resect_ref
import similarity_ref
import test_host_tables as tht
import track_ref
import tri_ransac_ref
import triangulate_ref
import two_view_ref


def test_the_catalogue_reaches_every_function_that_launches_work():
    from sfmba import _capi
    reached = {c for e in hh.ENTRIES.values() for c in e["calls"]}
    assert reached <= set(_capi.SIGNATURES)
    defaults = {name for name in _capi.SIGNATURES if name.startswith("sfmba_default_")}        # fill a structure on the host
    assert not reached & set(hh.NOT_IN_CATALOGUE) and not reached & set(hh.NO_WORK)
    assert set(hh.NOT_IN_CATALOGUE) | set(hh.NO_WORK) <= set(_capi.SIGNATURES)
    assert all(hh.NOT_IN_CATALOGUE.values())
    left = set(_capi.SIGNATURES) - reached - set(hh.NOT_IN_CATALOGUE) - set(hh.NO_WORK) - defaults
    assert not left, sorted(left)
    # the compute methods of the wrapper the issue names, each under its own name or with its variants
    for method in ("residuals", "residual_jacobian", "normal_blocks", "schur_matvec", "rhs_precond", "solve", "reprojection_stats",
                   "triangulate", "triangulate_ransac", "resect", "resect_ransac", "fundamental_ransac", "homography_ransac",
                   "essential_ransac", "similarity_ransac", "recover_pose", "match_descriptors", "build_tracks", "plan_views",
                   "assemble_problem"):
        assert method in hh.ENTRIES, method
    assert {"covariance_marginal", "covariance_conditional"} <= set(hh.ENTRIES)
    # a call with masks or optional outputs is there twice
    for name, e in hh.ENTRIES.items():
        assert e["masked"] in hh.ENTRIES and set(e["reads"]) <= {"problem", "descriptors", "tracks"}, name


def test_pairs_are_the_product_of_the_tables_minus_the_exclusions():
    assert len(hh.PAIRS) == len(hh.ENTRIES) * len(hh.PASTS) - len(hh.EXCLUDED)
    assert {p for _, p in hh.EXCLUDED} <= {"family", "family_reversed"}
    for fam in hh.FAMILIES:
        for name in fam:
            assert (name, "family") in hh.PAIRS and hh.siblings(name)
    # the orders the issue names
    assert hh.siblings("recover_pose") == ["similarity_ransac_masked", "fundamental_ransac_masked", "homography_ransac_masked",
                                           "essential_ransac_masked"]
    assert hh.siblings("triangulate") == ["triangulate_ransac_masked"] and hh.siblings("triangulate_ransac") == ["triangulate_masked"]
    assert hh.siblings("resect_masked") == ["resect_ransac_masked", "covariance_marginal", "covariance_conditional",
                                            "reprojection_stats_filtered"]


def camera_major(args):
    return np.argsort(np.asarray(args[2]), kind="stable")


def test_twin_has_the_sizes_of_the_entry_and_other_content():
    e, t = hh.inputs("entry"), hh.inputs("twin")
    assert hh.dims("entry") == hh.dims("twin")
    for name in ("tracks", "slices", "cov"):
        a, b = e[name]["args"], t[name]["args"]
        assert not np.array_equal(camera_major(a), camera_major(b)), name
        assert a[4].shape == b[4].shape and not np.array_equal(a[4], b[4]), name
        assert not np.array_equal(e[name]["x"], t[name]["x"])
    assert not np.array_equal(camera_major(e["ba"].args), camera_major(t["ba"].args))
    assert not np.array_equal(e["ba"].points_2d, t["ba"].points_2d)
    for name, keys in (("tracks", ("select", "use")), ("slices", ("select", "use", "samples")), ("fundamental", ("a", "b", "use", "samples")),
                       ("homography", ("a", "use", "samples")), ("essential", ("a", "use", "samples")), ("similarity", ("a", "use", "samples")),
                       ("pose", ("a", "use", "E")), ("trk", ("use",))):
        for k in keys:
            assert e[name][k].shape == t[name][k].shape and not np.array_equal(e[name][k], t[name][k]), (name, k)
    assert all(a.shape == b.shape and not np.array_equal(a, b) for a, b in zip(e["descs"], t["descs"]))
    assert all(a.shape == b.shape for a, b in zip(e["trk"]["batch"], t["trk"]["batch"]))
    assert not np.array_equal(e["trk"]["batch"][3], t["trk"]["batch"][3])


def test_larger_is_larger_and_smaller_is_smaller_in_every_dimension():
    e, lg, sm = hh.dims("entry"), hh.dims("larger"), hh.dims("smaller")
    same = {"descs.dim", "descs.dtype"}                         # the descriptor's length and type size no buffer by themselves
    for k in e:
        if k in same:
            assert e[k] == lg[k] == sm[k], k
        else:
            assert sm[k] < e[k] < lg[k], (k, sm[k], e[k], lg[k])


def test_entry_sizes_sit_on_both_sides_of_the_switches():
    I = hh.inputs("entry")
    for name in ("tracks", "cov"):
        runs = np.bincount(I[name]["args"][3])
        assert runs.min() < hh.LONG and hh.LONG in runs and runs.max() > hh.LONG, name
    per_cam = np.bincount(I["slices"]["args"][2])
    assert per_cam.min() < hh.CAM_STRIDE < per_cam.max()
    for kind, lds, slice_ in (("fundamental", hh.PAIR_LDS, hh.PAIR_SLICE), ("homography", hh.PAIR_LDS, hh.PAIR_SLICE),
                              ("essential", hh.PAIR_LDS, hh.PAIR_SLICE), ("similarity", hh.SIM_LDS, hh.SIM_SLICE)):
        n = np.diff(I[kind]["ptr"])
        assert n.min() < lds < n.max() and I[kind]["H"] > slice_, kind
    # the sample positions of every scale lie among the used members of their group
    for scale in hh.SCALES:
        J = hh.inputs(scale)
        for kind in ("fundamental", "homography", "essential", "similarity"):
            used = hh.used_per_group(J[kind]["ptr"], J[kind]["use"])
            assert np.all(J[kind]["samples"] >= 0) and np.all(J[kind]["samples"].max(axis=(1, 2)) < used), (scale, kind)
        c = J["slices"]
        used = np.bincount(c["args"][2][c["use"]], minlength=c["args"][0])
        assert np.all(c["samples"] >= 0) and np.all(c["samples"].max(axis=(1, 2)) < used), scale
    assert I["slices"]["H"] > hh.PNP_SLICE
    lengths = np.diff(track_ref.build_tracks_ref(*I["trk"]["batch"], conflicts=1)["track_ptr"])
    assert lengths.min() < hh.LONG and hh.LONG in lengths and lengths.max() > hh.LONG
    assert hh.inputs("entry")["ba"].n_cameras > 21              # the PCG path: the record of a solve can replay


@pytest.mark.parametrize("name", hh.SEQUENCES)
def test_sequence_steps_expect_the_reuse_the_table_build_defines(name):
    steps = hh.sequence(name)
    exp = tht.expected(hh.as_host_calls(steps))
    for k, (s, e) in enumerate(zip(steps, exp)):
        assert bool(e["ok"]) == s["ok"], (name, k)
        if s["ok"]:
            assert s["reuse"] == e["fdiff"], (name, k, s["note"], s["reuse"], e["fdiff"])
    if name == "reuse":
        N = len(steps[0]["cam"])
        assert [s["reuse"] for s in steps] == [0, N, N // 2, N, N - 40, N - 40, 0, N, 0] and [s["f32"] for s in steps[-3:]] == [1, 1, 0]
        assert N % 256 and (N - 40) % 256
    if name == "reuse_packed":
        assert all(s["packed"] for s in steps) and any(np.abs(s["uv"]).max() >= 32768 for s in steps)
    if name == "unsorted":
        assert [int(np.all(np.diff(s["pt"]) >= 0)) for s in steps] == [0, 1, 0]
    if name == "same_arrays":
        assert all(np.array_equal(s["cam"], steps[0]["cam"]) and s["uv"] is not None for s in steps)
        assert [s["fixed"] for s in steps[3:7]] == [(), (0,), (0, 3), ()] and all(s["consumers"] for s in steps[3:])
        assert not np.array_equal(steps[1]["K"], steps[0]["K"]) and steps[7]["C"] == steps[0]["C"] + 3


# ---- the restatements accept the inputs ----------------------------------------------------------------------------------------
def test_problem_consumers_inputs():
    I = hh.inputs("entry")
    t, c = I["tracks"], I["slices"]
    for kw in (dict(), dict(select=t["select"], obs_use=t["use"])):
        ref = triangulate_ref.triangulate(t["x"], t["args"], **kw)
        chosen = ref["status"] >= 0
        assert (ref["status"][chosen] == 0).mean() >= 0.9, np.bincount(ref["status"][chosen])
    ref = tri_ransac_ref.triangulate_ransac(t["x"], t["args"], select=t["select"], obs_use=t["use"], max_pairs=t["H"], seed=11)
    chosen = ref["status"] >= 0
    assert (ref["status"][chosen] == 0).mean() >= 0.9
    for kw in (dict(), dict(select=c["select"], obs_use=c["use"])):
        ref = resect_ref.resect(c["x"], c["args"], **kw)
        chosen = ref["status"] >= 0
        assert chosen.any() and np.all(ref["status"][chosen] == 0), ref["status"]
    ref = pnp_ransac_ref.resect_ransac(c["x"], c["args"], select=c["select"], obs_use=c["use"], samples=c["samples"], threshold=3.0)
    chosen = ref["status"] >= 0
    assert chosen.any() and np.all(ref["status"][chosen] == 0), ref["status"]
    from oracle import ba_oracle as orc
    for key in ("tracks", "slices", "cov"):
        assert np.isfinite(orc.compute_residuals(I[key]["x"], *I[key]["args"])).all()
    assert np.isfinite(orc.compute_residuals(I["ba"].x0, *I["ba"].args)).all()


def test_covariance_inputs():
    for scale in ("entry", "twin"):
        c = hh.inputs(scale)["cov"]
        for kind in (0, 1):
            ref = covariance_ref.covariance(c["x"], c["args"], kind=kind)
            assert ref["status"] == 0 and np.all(ref["pt_status"] == 0), (scale, kind, ref["status"])


def test_failing_inputs_reach_every_failing_status():
    I = hh.inputs("entry")
    seen = set()
    for x, kw in hh.failing_triangulations(I):
        seen |= set(triangulate_ref.triangulate(x, I["tracks"]["args"], **kw)["status"].tolist())
    assert {1, 2, 3, 4, 5} <= seen, seen                        # FEW_VIEWS, AT_INFINITY, BEHIND, LOW_ANGLE, HIGH_ERROR
    seen = set()
    for x, kw in hh.failing_resections(I):
        seen |= set(resect_ref.resect(x, I["slices"]["args"], **kw)["status"].tolist())
    assert {1, 2, 3, 4} <= seen, seen                           # FEW_VIEWS, DEGENERATE, BEHIND, HIGH_ERROR
    for case, status in (("c11_nogauge", 1), ("c3_undropped", 2)):
        c = covariance_ref.case(case)
        assert covariance_ref.covariance(c["x"], c["args"], gauge=c["gauge"])["status"] == status


def edges_of(p):
    ptr = p["ptr"]
    return [(e, slice(int(ptr[e]), int(ptr[e + 1]))) for e in range(len(ptr) - 1)]


def test_pair_model_inputs():
    I = hh.inputs("entry")
    calls = {"fundamental": lambda a, b, s: two_view_ref.ransac_edge(a, b, s, threshold=2.0, refit=True),
             "homography": lambda a, b, s: homography_ref.ransac_edge(a, b, s, threshold=2.0, refit=True),
             "essential": lambda a, b, s: essential_ref.ransac_edge(a, b, essential_ref.K_TEST, s, threshold=2.0),
             "similarity": lambda a, b, s: similarity_ref.ransac_set(a, b, s, 0.05, refit=True)}
    for kind, fn in calls.items():
        p = I[kind]
        for e, sl in edges_of(p):
            use = p["use"][sl]
            ref = fn(p["a"][sl][use], p["b"][sl][use], p["samples"][e][:16] if kind == "essential" else p["samples"][e])
            assert ref["status"] == 0 and ref["inliers"] >= (3 if kind == "similarity" else 8), (kind, e, ref["status"], ref["inliers"])
    p = I["pose"]
    for e, sl in edges_of(p):
        use = p["use"][sl]
        ref = two_view_ref.recover_pose_edge(p["E"][e], p["a"][sl][use], p["b"][sl][use], p["K"], min_depth=0.5)
        assert ref["status"] == 0, (e, ref["status"])


def test_matching_track_and_plan_inputs():
    I = hh.inputs("entry")
    ref = match_ref.match_batch(I["descs"], I["match_edges"], ratio=0.9)
    assert ref["n_ok"] == len(I["match_edges"]) and ref["good"].any()
    batch = I["trk"]["batch"]
    full = track_ref.build_tracks_ref(*batch, conflicts=1)
    cut = track_ref.build_tracks_ref(*batch, pair_use=I["trk"]["use"], min_length=3, max_length=12, conflicts=1)
    assert full["counts"]["tracks"] == len(hh.SIZES["entry"]["paths"]) and cut["counts"]["short"] > 0 and cut["counts"]["long"] > 0
    n_images, n_tracks = len(batch[0]) - 1, full["counts"]["tracks"]
    cam, trk = hh.plan_masks(I, n_images, n_tracks)
    views = plan_ref.plan_views_ref(full, cam, trk, img_ptr=batch[0])
    assert views["totals"]["ready"] > 0 and 0 < views["totals"]["known"] < n_tracks
    sub = plan_ref.assemble_ref(full, np.ones(n_images, bool), np.ones(n_tracks, bool), min_views=2, pts=np.concatenate(I["trk"]["kp"]),
                                img_ptr=batch[0])
    assert sub["counts"]["points"] == n_tracks
