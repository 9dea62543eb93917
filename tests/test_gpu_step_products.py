"""sfmba_step_products entry by entry in the forms no other test compares with a reference (tests/step_products_ref.py has
the references, the counts, the cases and the fp32 contract): k_jdot<false> and k_backsub<false> behind k_transpose (the
camera vector gathered from L2), the J-free instantiations, fp32 storage (load_blocks on the fp32 Jacobian, store_pair
and load_pair of t1, G11 from the unrounded and G12 from the stored t1), either side of the last camera count whose
vector fits the LDS, and the camera slice of k_backsub where it takes three trips.  One rank, every case a Backend of its
own; tests/test_host_step_products.py runs the same checks on an emulation and plants the errors they have to reject."""
import numpy as np
import pytest

import entry_bounds as eb
import step_products_ref as sp
from step_products_ref import CASES, JFREE_TWINS

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not eb.extended_precision(), reason="numpy.longdouble is no wider than a double on this machine")]

DEFAULTS = dict(dense=-1, vec_lds=-1, jfree=-1, sweep_rc=-1)


@pytest.fixture(scope="module")
def orc():
    from oracle import ba_oracle
    return ba_oracle


@pytest.fixture
def opened(orc):
    """opened(case name) -> (Backend, pb): a Backend of its own in the case's storage mode with its debug options, dense = 0,
    its held cameras and its problem set, the case's forms asserted; reset and closed when the test ends."""
    import sfmba
    made = []

    def open_(name):
        c = CASES[name]
        be = sfmba.Backend(0)
        made.append((be, ["dense"] + list(c["options"])))
        be.set_precision(c["bits"])
        be.debug_option("dense", 0)
        for option, value in c["options"].items():
            be.debug_option(option, value)
        be.set_fixed_cameras(c["fixed"])
        pb = sp.problem(c["problem"], orc)
        be.set_problem(*pb.args)
        got = {k: be.form(k) for k in c["forms"]}
        assert got == c["forms"], (name, got)
        if c["bits"] == 32:
            assert be.form("round_blocks") == (1 if c["options"].get("sweep_rc", -1) == 0 else 0), name
        return be, pb
    yield open_
    for be, names in made:
        for option in names:
            be.debug_option(option, DEFAULTS[option])
        be.close()


@pytest.mark.parametrize("name", list(CASES))
def test_entries_against_extended_precision(opened, orc, name):
    """t1, G11, dp and the ten sums of the case's form, each within its bound of the longdouble reference formed from the
    case's operands; in fp32 storage t1 is float32(reference) outside the tie entries, G11 sums the unrounded squares and
    G12 uses the stored t1."""
    be, pb = opened(name)
    _, case = sp.build_case(name, be, orc)
    sp._check_entries(be, pb, 0, case, name)


@pytest.mark.parametrize("name", list(JFREE_TWINS))
def test_jfree_form_has_the_bits_of_the_stored_form(opened, orc, name):
    """ba_kernels.hpp: the J-free consumers recompute an observation's blocks "as K1 itself forms them -- same function,
    same bits in fp64 storage": every output equals that of the stored form with the vector gathered from L2 (the same
    k_jdot<false, .> / k_backsub<false, .> but for the source of the blocks)."""
    be, pb = opened(name)
    _, case = sp.build_case(name, be, orc)                   # ONE set of sg, dc and diagonal for both handles
    a = be.step_products(pb.x0, case.sg, case.dc, case.diag)
    twin, _ = opened(JFREE_TWINS[name])
    b = twin.step_products(pb.x0, case.sg, case.dc, case.diag)
    seen = np.bincount(np.asarray(sp.problem(CASES[name]["problem"], orc).point_indices), minlength=a["dp"].shape[0]) > 0
    differ = {k: int(np.sum(a[k] != b[k])) for k in ("t1", "sums")}
    differ["dp"], differ["g11"] = int(np.sum(a["dp"][seen] != b["dp"][seen])), int(a["g11"] != b["g11"])
    print(f"{name} against {JFREE_TWINS[name]}: entries that differ {differ}")
    assert not any(differ.values()), (name, differ)


@pytest.mark.parametrize("name", ["64_l2vec_hand_built", "32_stored_l2vec_hand_built", "32_default_hand_built", "32_jfree_hand_built"])
def test_step_products_leaves_the_handle_as_it_found_it(opened, orc, name):
    """solve, step_products, solve: the second solve has the bits of the first, in both storages."""
    be, pb = opened(name)
    _, case = sp.build_case(name, be, orc)
    runs = []
    for call in (False, True):
        if call:
            be.step_products(pb.x0, case.sg, case.dc, case.diag)
        opt = be.default_options()
        opt.max_nfev = 6
        xs, res, fun, grad = be.solve(pb.x0, opt)
        runs.append((xs, fun, grad, res.nfev, res.cost, be.pcg_history()))
    a, b = runs
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3:] == b[3:], name
    # ... and of the solve on a handle that never made the call
    fresh, _ = opened(name)
    opt = fresh.default_options()
    opt.max_nfev = 6
    xs, res, fun, grad = fresh.solve(pb.x0, opt)
    assert np.array_equal(a[0], xs) and np.array_equal(a[1], fun) and np.array_equal(a[2], grad), name
    assert a[3:] == (res.nfev, res.cost, fresh.pcg_history()), name


def test_multi_rank_handle_is_still_refused_by_name(orc):
    """The single-rank refusal stays, also in fp32 storage: a handle with a transport attached (the callback transport
    over a world of one, whose all-reduce is the identity) has the several-rank forms."""
    import sfmba
    import torch
    pb = sp.problem("tiny", orc)
    be = sfmba.Backend(0)
    try:
        be.set_precision(32)
        be.set_problem(*pb.args)
        arena = torch.zeros(be.exchange_doubles(), dtype=torch.float64, device="cuda:0")
        be.set_exchange(arena.data_ptr(), arena.numel(), lambda dev_ptr, count, op: None, pb.n_obs)
        with pytest.raises(ValueError, match="sfmba_step_products is a single-rank entry"):
            be.step_products(pb.x0, np.ones(pb.x0.shape[0]), np.ones(6 * pb.n_cameras), np.ones(3 * pb.n_points))
        be.set_exchange(0, 0, None, 0)
        out = be.step_products(pb.x0, np.ones(pb.x0.shape[0]), np.ones(6 * pb.n_cameras), np.ones(3 * pb.n_points))
        assert np.array_equal(out["t1"].astype(np.float32), out["t1"])            # single rank again: served, float32 values
    finally:
        be.close()
