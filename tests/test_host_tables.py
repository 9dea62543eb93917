"""The host's table build of sfmba_set_problem (csrc/problem_tables.hpp), run without a device under the host sanitizers.

tests/host/problem_tables_check.cpp calls the same code the library calls; the Makefile builds it twice, with
AddressSanitizer + UndefinedBehaviorSanitizer and with ThreadSanitizer.  Every case runs under both as a subprocess, must
end with status 0 and an empty stderr, and its output is compared with `expected()` below: a numpy restatement written
from the definitions of the tables ("The table build without a device"), not from the C++.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

PKG = os.path.join(ROOT, "sfm-python_amd")
RUN_SECONDS = 60

PLAN = dict(dense=0, xcd_b=0, cm_device=0, packed_upload=0, cam_chunk_len=4096, total_waves=4, parts=1, pair_parts=1)
# the arrays of the output file, in its order
ARRAYS = (("ptr", "<i4", 1), ("perm", "<i4", 1), ("order", "<i8", 1), ("cam_ptr", "<i4", 1), ("ranges", "<i4", 2), ("wsteps", "<i4", 2),
          ("steps", "<i4", 2), ("chunks", "<i4", 4), ("chunk_ptr", "<i4", 1), ("chunks_b", "<i4", 4), ("chunk_ptr_b", "<i4", 1),
          ("cov_ptr", "<i4", 1), ("cov_pt", "<i4", 1), ("blk_ab", "<i4", 2), ("ci", "<i4", 1), ("pi", "<i4", 1), ("uvs", "<f8", 2),
          ("uvf", "<f4", 2), ("ci16", "<u2", 1), ("uv16", "<i2", 2))
SCALARS = ("ok", "bad", "sorted", "fdiff", "pixels_int16", "cam_multi", "pair_entries", "ld")


def call(C, P, cam, pt, uv, fixed=(), f32=0, **plan):
    unknown = set(plan) - set(PLAN)
    assert not unknown, unknown
    return dict(C=C, P=P, cam=np.asarray(cam, np.int64), pt=np.asarray(pt, np.int64), uv=np.asarray(uv), fixed=list(fixed), f32=f32,
                plan=dict(PLAN, **plan))


def write_cases(path, calls):
    with open(path, "wb") as f:
        np.array([len(calls)], "<i8").tofile(f)
        for c in calls:
            p = c["plan"]
            i64 = c["uv"].dtype.kind == "i"
            np.array([c["C"], c["P"], len(c["cam"]), len(c["fixed"]), i64, c["f32"], p["dense"], p["xcd_b"], p["cm_device"],
                      p["packed_upload"], p["cam_chunk_len"], p["total_waves"], p["parts"], p["pair_parts"]], "<i8").tofile(f)
            c["cam"].astype("<i8").tofile(f)
            c["pt"].astype("<i8").tofile(f)
            c["uv"].astype("<i8" if i64 else "<f8").tofile(f)
            np.array(c["fixed"], "<i8").tofile(f)


def read_output(path, n_calls):
    buf = open(path, "rb").read()
    at, out = 0, []
    for _ in range(n_calls):
        rec = dict(zip(SCALARS, (int(v) for v in np.frombuffer(buf, "<i8", 8, at))))
        at += 64
        if rec["ok"]:
            for name, dtype, width in ARRAYS:
                n = int(np.frombuffer(buf, "<i8", 1, at)[0])
                rec[name] = np.frombuffer(buf, dtype, n, at + 8).reshape(-1, width) if width > 1 else np.frombuffer(buf, dtype, n, at + 8)
                at += 8 + n * np.dtype(dtype).itemsize
        out.append(rec)
    assert at == len(buf)
    return out


# ---- the definitions, restated ------------------------------------------------------------------------------------------
def expected(calls):
    """What every call of a sequence on one staging must give; `prev` is the stored problem a call is compared with."""
    out, prev = [], None
    for c in calls:
        e = expected_one(c, prev)
        out.append(e)
        # only a completed, point-major call leaves something to compare the next one with
        prev = dict(f32=c["f32"], cam=e["ci"][:e["N"]], pt=e["pi"][:e["N"]], uv=e["uvs"][:e["N"]]) if e["ok"] and e["sorted"] else None
    return out


def expected_one(c, prev):
    C, P, plan = c["C"], c["P"], c["plan"]
    cam, pt, uv = c["cam"], c["pt"], c["uv"].reshape(-1, 2)
    N = len(cam)
    ld = (N + 255) // 256 * 256
    wrong = np.flatnonzero((cam < 0) | (cam >= C) | (pt < 0) | (pt >= P))
    if len(wrong):
        return dict(ok=0, bad=int(wrong[0]), N=N)
    e = dict(ok=1, bad=-1, N=N, ld=ld)
    e["sorted"] = int(np.all(np.diff(pt) >= 0))
    e["order"] = np.zeros(0, np.int64) if e["sorted"] else np.argsort(pt, kind="stable")
    if not e["sorted"]:
        cam, pt, uv = cam[e["order"]], pt[e["order"]], uv[e["order"]]
    uvd = uv.astype(np.float64)
    pad = lambda a, dtype: np.concatenate([a, np.zeros((ld - N,) + a.shape[1:], a.dtype)]).astype(dtype)
    e["ci"], e["pi"], e["uvs"] = pad(cam, np.int32), pad(pt, np.int32), pad(uvd, np.float64)
    e["uvf"] = pad(uvd, np.float32) if c["f32"] else np.zeros((0, 2), np.float32)
    is16 = bool(np.all((uvd == np.rint(uvd)) & (np.abs(uvd) < 32768)))
    if plan["packed_upload"]:
        e["pixels_int16"] = int(is16)
        if is16:
            e["ci16"], e["uv16"] = pad(cam, np.uint16), pad(uvd, np.int16)
    # first stored observation that differs from the previous problem's
    e["fdiff"] = 0
    if prev is not None and prev["f32"] == c["f32"] and e["sorted"]:
        n = min(len(prev["cam"]), N)
        differs = (prev["cam"][:n] != cam[:n]) | (prev["pt"][:n] != pt[:n]) | np.any(prev["uv"][:n] != uvd[:n], axis=1)
        e["fdiff"] = int(np.flatnonzero(differs)[0]) if differs.any() else n
    e["ptr"] = np.searchsorted(pt, np.arange(P + 1), side="left").astype(np.int32)          # observations whose point is < p
    held = np.zeros(C, bool)
    held[c["fixed"]] = True
    free = np.flatnonzero(~held[cam])                                                      # stored positions of the cameras that move
    e["cam_ptr"] = np.concatenate([[0], np.cumsum(np.bincount(cam[free], minlength=C))]).astype(np.int32)
    perm = free[np.argsort(cam[free], kind="stable")]
    if not plan["cm_device"]:
        e["perm"] = np.concatenate([perm, np.zeros(ld - len(perm), np.int64)]).astype(np.int32)
    else:
        e["perm"] = np.zeros(0, np.int32)
    ptr = e["ptr"].astype(np.int64)

    # wave ranges: greedy, closed at the first point boundary with >= T observations; the last takes the remainder
    T = max(64, -(-N // plan["total_waves"]))
    ranges, start = [], 0
    for p in range(P):
        if ptr[p + 1] - start >= T or (p == P - 1 and ptr[p + 1] > start):
            ranges.append((start, ptr[p + 1]))
            start = ptr[p + 1]
    e["ranges"] = np.array(ranges, np.int32).reshape(-1, 2)
    # steps: a point of more than 64 observations is one step; else up to the largest point boundary <= pos + 64 inside the range
    steps, wsteps = [], []
    for b, end in ranges:
        first, pos = len(steps), b
        while pos < end:
            run_end = ptr[pt[pos] + 1]
            if run_end - pos > 64:
                cut = run_end
            else:
                bounds = ptr[ptr <= min(pos + 64, end)]
                cut = bounds.max()
            assert pos < cut <= end
            steps.append((pos, cut - pos))
            pos = cut
        wsteps.append((first, len(steps) - first))
    e["steps"], e["wsteps"] = np.array(steps, np.int32).reshape(-1, 2), np.array(wsteps, np.int32).reshape(-1, 2)

    # chunks of the camera-major lists
    L = plan["cam_chunk_len"]
    chunks, chunk_ptr = [], [0]
    for k in range(C):
        b, end = int(e["cam_ptr"][k]), int(e["cam_ptr"][k + 1])
        n = max(1, -(-(end - b) // L))
        chunks += [(k, min(end, b + j * L), min(end, b + (j + 1) * L), n) for j in range(n)]
        chunk_ptr.append(len(chunks))
    e["chunks"], e["chunk_ptr"] = np.array(chunks, np.int32), np.array(chunk_ptr, np.int32)
    e["cam_multi"] = int(any(row[3] > 1 for row in chunks))
    e["chunk_ptr_b"] = np.zeros(0, np.int32)
    if plan["xcd_b"]:
        tab = np.tile(np.array([-1, 0, 0, 8], np.int32), ((C + 3) // 4 * 8 * 4, 1))
        for k in range(C if not plan["cm_device"] else 0):
            b, end = int(e["cam_ptr"][k]), int(e["cam_ptr"][k + 1])
            pts = pt[perm[b:end]]
            for r in range(8):
                lo, hi = P * r // 8, P * (r + 1) // 8
                tab[((k // 4) * 8 + r) * 4 + k % 4] = (k, b + np.count_nonzero(pts < lo), b + np.count_nonzero(pts < hi), 8)
        e["chunks_b"] = tab
    else:
        e["chunks_b"] = np.zeros((0, 4), np.int32)

    # pair lists of the dense path: per block (a <= b) of cameras that move, the points both see, with multiplicity
    e["pair_entries"] = 0
    e["cov_ptr"], e["blk_ab"], e["cov_lists"] = np.zeros(0, np.int32), np.zeros((0, 2), np.int32), []
    if plan["dense"]:
        seen = np.zeros((C, P), np.int64)                         # how often camera c sees point p
        np.add.at(seen, (cam[free], pt[free]), 1)
        blocks = [(a, b) for a in range(C) for b in range(a, C)]
        lists = []
        for a, b in blocks:
            if a != b:
                lists.append(np.repeat(np.arange(P), seen[a] * seen[b]))
            else:               # every observation with itself once, as ~p; every unordered pair of distinct ones twice
                m = seen[a]
                both = np.concatenate([np.repeat(~np.arange(P), m), np.repeat(np.arange(P), m * (m - 1))])
                lists.append(both[np.argsort(np.where(both < 0, ~both, both), kind="stable")])
        e["cov_lists"] = lists
        e["cov_ptr"] = np.concatenate([[0], np.cumsum([len(v) for v in lists])]).astype(np.int32)
        e["pair_entries"] = int(e["cov_ptr"][-1])
        e["blk_ab"] = np.array(blocks, np.int32)
    return e


def compare(got, exp, tag):
    for name in ("ok", "bad"):
        assert got[name] == exp[name], (tag, name, got[name], exp[name])
    if not exp["ok"]:
        return
    for name in ("sorted", "fdiff", "cam_multi", "pair_entries", "ld") + (("pixels_int16",) if "pixels_int16" in exp else ()):
        assert got[name] == exp[name], (tag, name, got[name], exp[name])
    for name, _, _ in ARRAYS:
        if name == "cov_pt" or name not in exp:
            continue
        assert got[name].shape == exp[name].shape and np.array_equal(got[name], exp[name]), (tag, name, got[name], exp[name])
    # a block's list: ascending in the point; inside a point the order of p and ~p entries is the implementation's
    for k, want in enumerate(exp["cov_lists"]):
        have = got["cov_pt"][exp["cov_ptr"][k]:exp["cov_ptr"][k + 1]]
        point = np.where(have < 0, ~have, have)
        assert np.all(np.diff(point) >= 0), (tag, "cov_pt order", k)
        assert np.array_equal(np.sort(have), np.sort(want)), (tag, "cov_pt", k, have, want)


# ---- cases --------------------------------------------------------------------------------------------------------------
def point_major(rng, C, lens, cams_of=None):
    """Observation arrays of tracks of the given lengths, in point-major order, with pixels of a quarter-pixel grid."""
    pt = np.repeat(np.arange(len(lens)), lens)
    cam = np.concatenate([cams_of(n) if cams_of else rng.integers(0, C, n) for n in lens] + [np.zeros(0, np.int64)]).astype(np.int64)
    uv = rng.integers(-4000, 4000, (len(pt), 2)) / 4.0
    return cam, pt, uv


def boundary_problem(C=9):
    """Ragged runs, point 17 never observed, camera C - 1 never observed, one (camera, point) pair twice, cameras 0 and 2 held."""
    rng = np.random.default_rng(3)
    lens = np.minimum(rng.integers(1, 6, 60), C - 1)
    lens[[3, 17, 30, 59]] = [1, 0, C - 1, 2]
    cam, pt, uv = point_major(rng, C, lens, lambda n: rng.permutation(C - 1)[:n])
    k = int(np.flatnonzero(pt == 30)[0])
    cam[k + 1] = cam[k]
    assert C - 1 not in cam and 17 not in pt and 0 in cam and 2 in cam
    return dict(C=C, P=60, cam=cam, pt=pt, uv=uv, fixed=(0, 2))


@functools.lru_cache(maxsize=None)
def case(name):
    rng = np.random.default_rng(sum(name.encode()))
    if name == "boundary":                          # (a)
        return [call(dense=1, xcd_b=x, **boundary_problem(C)) for C, x in ((9, 0), (5, 1), (21, 0))]
    if name == "step_edges":                        # (b)
        lens = np.concatenate([[1, 63, 64, 65, 128, 130], rng.integers(1, 5, 10), [64, 1, 63, 2], [100]])
        cam, pt, uv = point_major(rng, 12, lens)
        assert 600 <= len(pt) <= 800
        return [call(12, len(lens), cam, pt, uv, dense=1, total_waves=4)]
    if name == "unsorted":                          # (c)
        b = boundary_problem()
        sh = np.random.default_rng(8).permutation(len(b["pt"]))
        shuffled = dict(b, cam=b["cam"][sh], pt=b["pt"][sh], uv=b["uv"][sh])
        # ... also behind a point-major call (nothing is re-used on this path), with a packed plan, in two parts
        return [call(dense=1, **shuffled), call(dense=1, **b), call(dense=1, parts=2, packed_upload=1, **dict(shuffled, uv=np.rint(shuffled["uv"])))]
    if name == "parts":                             # (d)
        lens = rng.integers(5, 14, 100)
        lens[-1] += 1000 - lens.sum()
        cam, pt, uv = point_major(rng, 15, lens)
        ptr = np.concatenate([[0], np.cumsum(lens)])
        assert len(pt) == 1000 and lens.min() > 0 and not {500, 334, 668, 200, 400}.issubset(ptr)
        return [call(15, 100, cam, pt, np.rint(uv), fixed=(2,), dense=1, xcd_b=1, packed_upload=1, parts=n) for n in (1, 2, 3, 5)]
    if name == "pair_threads":                      # (e)
        cam, pt, uv = point_major(rng, 8, rng.integers(0, 7, 50))
        return [call(8, 50, cam, pt, uv, fixed=(1,), dense=1, pair_parts=n) for n in (1, 4)]
    if name == "parallel_steps":                    # (f)
        lens = rng.integers(1, 8, 5000)
        lens[[10, 2500, 4999]] = [70, 64, 200]
        cam, pt, uv = point_major(rng, 30, lens)
        assert 19000 <= len(pt) <= 21000
        return [call(30, 5000, cam, pt, uv, total_waves=256, parts=n) for n in (1, 3)]
    if name == "chunking":                          # (g)
        calls = []
        for C in (1, 4, 5, 9):
            for P in (8, 13):
                counts = np.concatenate([[30, 10, 5, 0], rng.integers(0, 20, 5)])[:C]
                cam = np.repeat(np.arange(C), counts)
                pt = rng.integers(0, P, len(cam))
                pt[0], pt[1] = 0, P - 1
                o = np.argsort(pt, kind="stable")
                uv = rng.integers(-4000, 4000, (len(cam), 2)) / 4.0
                calls += [call(C, P, cam[o], pt[o], uv, dense=1, xcd_b=1, cm_device=d, cam_chunk_len=7) for d in (0, 1)]
        return calls
    if name in ("reuse", "reuse_packed"):           # (h)
        packed = name == "reuse_packed"
        lens = rng.integers(1, 7, 150)
        cam, pt, uv = point_major(rng, 10, lens)
        uv = np.rint(uv).astype(np.int64) if packed else uv
        N, mid = len(pt), len(pt) // 2
        changed = uv.copy()
        changed[mid, 1] += 1
        more = rng.integers(1, 5, 20)
        cam2, pt2, uv2 = point_major(rng, 10, more)
        grown = (np.concatenate([cam, cam2]), np.concatenate([pt, pt2 + 150]), np.concatenate([changed, uv2.astype(uv.dtype)]))
        make = lambda P, cam, pt, uv, **kw: call(10, P, cam, pt, uv, dense=1, packed_upload=int(packed), parts=2, **kw)
        calls = [make(150, cam, pt, uv), make(150, cam, pt, uv), make(150, cam, pt, changed), make(170, *grown),
                 make(150, cam[:N - 40], pt[:N - 40], changed[:N - 40]), make(150, cam, pt, changed)]
        if packed:
            far = changed.copy()
            far[mid + 3, 0] = 40000
            calls += [make(150, cam, pt, far), make(150, cam, pt, far), make(150, cam, pt, changed)]
        else:           # a change of the storage precision re-uses nothing; the next call in that precision does
            calls += [make(150, cam, pt, changed, f32=1), make(150, cam, pt, changed, f32=1)]
        return calls
    if name == "bad_index":                         # (i)
        b = boundary_problem()
        cam_bad, pt_bad = b["cam"].copy(), b["pt"].copy()
        cam_bad[100], pt_bad[[41, 120]] = b["C"], (-1, 60)
        return [call(dense=1, **b), call(dense=1, parts=2, **dict(b, cam=cam_bad)), call(dense=1, **b),
                call(dense=1, packed_upload=1, **dict(b, pt=pt_bad)), call(dense=1, **b)]
    raise KeyError(name)


CASES = ("boundary", "step_edges", "unsorted", "parts", "pair_threads", "parallel_steps", "chunking", "reuse", "reuse_packed", "bad_index")


@functools.lru_cache(maxsize=None)
def expected_of(name):
    return expected(case(name))


@pytest.fixture(scope="module")
def binaries():
    subprocess.run(["make", "-C", PKG, "host-check"], check=True, capture_output=True, timeout=600)
    return {k: os.path.join(PKG, "build", "problem_tables_check_" + k) for k in ("asan", "tsan")}


@pytest.mark.parametrize("sanitizer", ["asan", "tsan"])
@pytest.mark.parametrize("name", CASES)
def test_tables_under_sanitizers_equal_their_definitions(binaries, tmp_path, name, sanitizer):
    calls = case(name)
    write_cases(tmp_path / "cases.bin", calls)
    run = subprocess.run([binaries[sanitizer], str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True,
                         timeout=RUN_SECONDS)
    assert run.returncode == 0 and run.stderr == "", (run.returncode, run.stderr[-4000:])
    got = read_output(tmp_path / "out.bin", len(calls))
    for k, (g, e) in enumerate(zip(got, expected_of(name))):
        compare(g, e, (name, k))
    # the same problem on other thread counts: every output identical (but the re-used prefix: the later calls repeat the first)
    if name in ("parts", "pair_threads", "parallel_steps"):
        for g in got[1:]:
            for key in set(got[0]) - {"fdiff"}:
                assert np.array_equal(g[key], got[0][key]), (name, key)


def test_the_cases_reach_their_branches():
    """The structure the cases were chosen for is there (by the expected tables: nothing is run)."""
    e = expected_of("step_edges")[0]
    assert {1, 63, 64, 65, 128, 130} <= set(np.diff(e["ptr"])) and len(e["ranges"]) > 1
    assert any(n > 64 for _, n in e["steps"]) and any(n == 64 for _, n in e["steps"])
    e = expected_of("parallel_steps")[0]
    assert len(e["ranges"]) // 64 >= 2
    for e, c in zip(expected_of("chunking"), case("chunking")):
        per_cam = np.diff(e["chunk_ptr"])
        assert e["cam_multi"] and per_cam.max() > 2
        if c["C"] >= 4:
            assert {1, 2} <= set(per_cam) and np.any(np.diff(e["cam_ptr"]) == 0)
    N = expected_of("reuse")[0]["N"]
    assert [e["fdiff"] for e in expected_of("reuse")] == [0, N, N // 2, N, N - 40, N - 40, 0, N]
    N = expected_of("reuse_packed")[0]["N"]
    assert [e["fdiff"] for e in expected_of("reuse_packed")] == [0, N, N // 2, N, N - 40, N - 40, N // 2 + 3, N, N // 2 + 3]
    assert [e["pixels_int16"] for e in expected_of("reuse_packed")] == [1, 1, 1, 1, 1, 1, 0, 0, 1]
    assert [(e["ok"], e["bad"]) for e in expected_of("bad_index")] == [(1, -1), (0, 100), (1, -1), (0, 41), (1, -1)]
    assert [e.get("fdiff") for e in expected_of("bad_index")] == [0, None, 0, None, 0]
    assert [e["sorted"] for e in expected_of("unsorted")] == [0, 1, 0] and expected_of("unsorted")[2]["fdiff"] == 0
