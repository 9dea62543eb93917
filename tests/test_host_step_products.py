"""tests/step_products_ref.py without a GPU: k_jdot and k_backsub emulated in plain float64 numpy (Emulation: the fp32
roundings of the named operands, the device's summation structure) lie inside every bound of every case of
test_gpu_step_products.py, the conditions that keep those bounds meaningful hold, and six planted errors are each
rejected by a named check -- three of them errors that the 1e-6-of-the-largest-entry window, the only normwise standard
fp32 storage has elsewhere, accepts."""
import numpy as np
import pytest

import entry_bounds as eb
import step_products_ref as sp
from step_products_ref import CASES, SUM_NAMES, Emulation

pytestmark = pytest.mark.skipif(not eb.extended_precision(), reason="numpy.longdouble is no wider than a double on this machine")

CAMERA_SUMS = SUM_NAMES[7:]


@pytest.fixture(scope="module")
def orc():
    from oracle import ba_oracle
    return ba_oracle


_made = {}


def _emulated(name, orc, plant=None):
    """-> (Emulation, pb, case, out) of a case; the unplanted emulation and its _Case are built once per case."""
    c = CASES[name]
    pb = sp.problem(c["problem"], orc)
    if name not in _made:
        em = Emulation(orc, pb, c["bits"], c["options"], c["fixed"])
        _made[name] = (em, sp.build_case(name, em, orc)[1])
    case = _made[name][1]
    em = _made[name][0] if plant is None else Emulation(orc, pb, c["bits"], c["options"], c["fixed"], plant)
    return em, pb, case, em.step_products(pb.x0, case.sg, case.dc, case.diag)


def _rejected(name, orc, plant):
    em, pb, case, out = _emulated(name, orc, plant)
    ok, fig, _ = sp.judge(out, 0, case)
    print(f"{name} with {plant}: {fig}")
    return {k for k, v in ok.items() if not v}, out, case


def _window(got, ref):
    """The normwise standard: within 1e-6 of the largest entry."""
    return eb.rel_max(np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)) <= 1e-6


@pytest.mark.parametrize("name", list(CASES))
def test_emulation_inside_every_bound_and_the_bounds_mean_something(orc, name):
    """_check_entries, the check of the GPU tests, on the emulation: every entry and sum inside its bound, the tie cap, and
    SHARE / LEVEL: nine digits below 99 % of the entries and below every sum, with the reference alone."""
    em, pb, case, _ = _emulated(name, orc)
    assert {k: em.form(k) for k in CASES[name]["forms"]} == CASES[name]["forms"], name
    sp._check_entries(em, pb, 0, case, name)


def test_the_cases_reach_their_branches(orc):
    """hand_built: complete-run windows and the long-run step (runs of 65, 128, 256, 300: four of them, the last with a
    partial trip); 3370 cameras over 8000 observations: 7 workgroups, 2889 slice elements each, three trips."""
    em, _, _, _ = _emulated("64_l2vec_hand_built", orc)
    assert em.long_runs == 4 and len(em.ranges) > em.long_runs and 300 % 64 != 0 and eb.HAND_RUNS[-1] == 300
    em, _, _, _ = _emulated("64_last_lds_vec", orc)
    # (ranges of at least 64 observations cut at point boundaries: 7 workgroups, not the 8 that 8000 / 64 / 16 would give)
    assert sp.VEC == 3370 and (em.pb.n_cameras, em.grid, em.per, em.slice_trips) == (3370, 7, 2889, 3)
    assert (em.form("lds_vec"), _emulated("64_first_l2_vec", orc)[0].form("lds_vec")) == (1, 0)


FP32_STORED = [n for n, c in CASES.items() if c["bits"] == 32]


@pytest.mark.parametrize("name", FP32_STORED)
def test_plant_g11_from_the_stored_t1(orc, name):
    """G11 = sum float32(t1)^2: rejected by the G11 check alone; 1e-6 of its value accepts it."""
    bad, out, case = _rejected(name, orc, "g11_from_stored_t1")
    assert bad == {"G11"}, (name, bad)
    ref, _ = case.sums(out, 0)
    assert _window([out["g11"]], [ref[0]]), name


@pytest.mark.parametrize("name", FP32_STORED)
def test_plant_g12_from_the_unrounded_t1(orc, name):
    """G12 = sum t1 . t2 with the fp64 t1 instead of the stored one: rejected by the G12 check alone."""
    bad, out, case = _rejected(name, orc, "g12_from_unrounded_t1")
    assert bad == {"G12"}, (name, bad)
    ref, _ = case.sums(out, 0)
    assert _window([out["sums"][0]], [ref[1]]), name


@pytest.mark.parametrize("name", ["32_stored_hand_built", "32_first_l2_vec", "64_l2vec_hand_built", "64_jfree_hand_built"])
def test_plant_t_accumulated_in_fp32(orc, name):
    """t = Jc . dc accumulated in fp32: dp and G22 (t2) leave their bounds; t1 and G11 (k_jdot) do not see it; the normwise
    window accepts dp and every sum."""
    bad, out, case = _rejected(name, orc, "t_in_fp32")
    assert {"dp", "G22"} <= bad and not bad & ({"t1", "G11", "finite"} | set(CAMERA_SUMS)), (name, bad)
    ref, _ = case.sums(out, 0)
    assert _window(out["dp"][case.seen], case.dp[case.seen]), name
    assert all(_window([g], [r]) for g, r in zip(np.concatenate([[out["g11"]], out["sums"]]), ref)), name


@pytest.mark.parametrize("name", ["64_l2vec_hand_built", "32_stored_hand_built", "32_jfree_hand_built", "64_l2vec_rc_hand_built"])
def test_plant_last_partial_trip_of_a_long_run_dropped(orc, name):
    """The n_take == 0 step without the tail of the 300-long run (of the 200-long run of the older hand-built problem,
    whose test in test_gpu_rc_consumers.py catches the plant too): that point's dp and the Gram sums."""
    bad, out, case = _rejected(name, orc, "long_run_tail_dropped")
    assert {"dp", "G12", "G22"} <= bad and "t1" not in bad, (name, bad)
    wrong = np.abs(out["dp"].astype(eb.LD) - case.dp)[case.seen] > case.B_dp[0][case.seen]
    L = case.L[case.seen]
    partial = (L > 64) & (L % 64 != 0)                       # 65 and 300 of hand_built (128 and 256 are whole trips); 200
    assert partial[np.argmax(L)] and np.array_equal(wrong.any(axis=1), partial), name


@pytest.mark.parametrize("name", ["64_last_lds_vec", "32_last_lds_vec", "64_first_l2_vec", "32_first_l2_vec"])
def test_plant_camera_slice_after_its_first_trip_skipped(orc, name):
    """Only q5 .. q8 of the cameras move, and every one of them leaves its bound."""
    bad, _, _ = _rejected(name, orc, "camera_slice_one_trip")
    assert bad == set(CAMERA_SUMS), (name, bad)


def test_older_step_products_cases_cannot_see_the_camera_slice_plant(orc):
    """The cases of test_gpu_rc_consumers.py (and every other case here): a workgroup's share of the camera slice is at most
    its 1024 threads, the loop takes one trip, and the planted kernel is the kernel."""
    import sfmba
    old = {"tiny": sp.problem("tiny", orc), "medium": sfmba.make_problem(60, 900, 9000, seed=12),
           "hand_built": sp.problem("rc_hand_built", orc), "gaps": sp.problem("gaps", orc),
           "1100 cameras": sfmba.make_problem(1100, 1500, 12000, seed=8), "1101 cameras": sfmba.make_problem(1101, 1500, 12000, seed=8)}
    for tag, pb in old.items():
        em = Emulation(orc, pb, plant="camera_slice_one_trip")
        assert em.per <= 1024, (tag, em.per)
    for name, c in CASES.items():
        if not c["problem"].startswith("schur_"):
            assert _emulated(name, orc)[0].per <= 1024, name
    _, _, _, a = _emulated("64_l2vec_rc_hand_built", orc)
    _, _, _, b = _emulated("64_l2vec_rc_hand_built", orc, "camera_slice_one_trip")
    assert np.array_equal(a["sums"], b["sums"]) and a["g11"] == b["g11"]


@pytest.mark.parametrize("name", ["64_l2vec_hand_built", "64_first_l2_vec", "32_stored_l2vec_hand_built", "32_first_l2_vec",
                                  "64_jfree_tiny"])
def test_plant_l2_vector_read_in_plane_major_order(orc, name):
    """The forms that gather the step from L2 reading it as if k_transpose had not run: dp, the Gram sums and the cameras'
    sums (the slice pairs the step with the wrong gradient entries) leave their bounds; k_jdot's outputs stay."""
    bad, _, _ = _rejected(name, orc, "plane_major_dc")
    assert {"dp", "G12", "G22", "q5 cameras", "q7 cameras"} <= bad and not bad & {"t1", "G11", "finite"}, (name, bad)


def test_plane_major_plant_is_invisible_to_the_lds_form(orc):
    """k_backsub<true> transposes the planes itself while it stages them: the cases with vec_lds = 0 are the ones that see it."""
    _, _, _, a = _emulated("64_last_lds_vec", orc)
    _, _, _, b = _emulated("64_last_lds_vec", orc, "plane_major_dc")
    assert np.array_equal(a["sums"], b["sums"]) and np.array_equal(a["dp"], b["dp"], equal_nan=True)
