"""tests/entry_bounds.py without a GPU: the conditions that keep the bounds of test_gpu_entries.py meaningful hold for
every one of its cases, the longdouble references agree with the fp64 oracle to the oracle's own rounding, and the
per-entry check rejects what the normwise check of test_gpu_parity.py lets through."""
import numpy as np
import pytest

import entry_bounds as eb

pytestmark = pytest.mark.skipif(not eb.extended_precision(), reason="numpy.longdouble is no wider than a double on this machine")


@pytest.fixture(scope="module")
def orc():
    from oracle import ba_oracle
    return ba_oracle


def _share(tag, what, ref, k, A, level=eb.LEVEL, share=eb.SHARE):
    bnd = eb.bound(k, A)
    s = eb.share_below(bnd, ref, level)
    assert np.all(np.isfinite(np.asarray(bnd, dtype=np.float64))) and np.all(bnd >= 0), (tag, what)
    assert s >= share, (tag, what, s)
    return s


@pytest.mark.parametrize("name", list(eb.K1_CASES))
def test_k1_cases_keep_their_bounds_nine_digits_below_the_entries(orc, name):
    problem, _, _ = eb.K1_CASES[name]
    lin = eb.linearisation(problem, orc)
    for what, ref, k, A in (("r", lin.r, lin.k_r, lin.ra), ("Jc", lin.Jc, lin.k_jc, lin.Jca), ("Jp", lin.Jp, lin.k_jp, lin.Jpa)):
        _share(name, what, ref, k, A)


@pytest.mark.parametrize("name", list(eb.BLOCK_CASES))
def test_block_cases(orc, name):
    problem, options, _ = eb.BLOCK_CASES[name]
    lin, st = eb.linearisation(problem, orc), eb.structure(problem, orc, options)
    b = lin.blocks(st)
    for q in ("U", "V", "gc", "gp"):
        _share(name, q, b[q], b["k_" + q], b[q + "a"])


@pytest.mark.parametrize("name", list(eb.RHS_CASES))
def test_rhs_cases(orc, name):
    problem, options, _ = eb.RHS_CASES[name]
    lin, st = eb.linearisation(problem, orc), eb.structure(problem, orc, options)
    dc, dp, _ = eb.operands(lin, st)
    ref = lin.rhs_pass(st, dc, dp)
    _share(name, "rhs", ref["rhs"], ref["k_rhs"], ref["rhsa"])
    _share(name, "sd", eb.upper(ref["sd"]), ref["k_sd"], eb.upper(ref["sda"]))
    s = _share(name, "minv", eb.upper(ref["minv"]), ref["k_minv"], eb.upper(ref["minva"]), share=eb.SHARE_MINV)
    assert abs(s - 0.977) < 0.005, s                                   # the measured figure beside SHARE_MINV
    assert np.allclose(np.asarray(np.einsum("cij,cjk->cik", ref["M"], ref["minv"]), dtype=np.float64), np.eye(6), atol=1e-12)


@pytest.mark.parametrize("name", list(eb.SCHUR_CASES))
def test_schur_cases(orc, name):
    problem, options, _, pass_a = eb.SCHUR_CASES[name]
    lin, st = eb.linearisation(problem, orc), eb.structure(problem, orc, options)
    dc, dp, v = eb.operands(lin, st)
    ref = lin.schur_product(st, dc, dp, v, pass_a)
    _share(name, "y", ref["y"], ref["k_y"], ref["ya"], level=eb.LEVEL_Y)


def test_dense_case(orc):
    problem = "dense_%d" % eb.DENSE_CAMERAS
    lin, st = eb.linearisation(problem, orc), eb.structure(problem, orc, {})
    assert lin.C == 21 and 6 * (lin.C + 1) > 128
    dc, dp, v = eb.operands(lin, st)
    ref = lin.dense_s(st, dc, dp)
    _share(problem, "S", ref["S"], ref["k_S"], ref["Sa"], level=eb.LEVEL_Y)
    y = lin.schur_product(st, dc, dp, v, "rc")["y"]                # the explicit matrix and the implicit product agree
    assert np.abs(np.asarray(ref["S"] @ v.astype(eb.LD) - y.ravel(), dtype=np.float64)).max() <= 1e-15 * float(np.abs(y).max())


def test_camera_counts_of_the_form_switches():
    from kernel_source import kernel_constant
    assert eb.lds_limit(kernel_constant("kCamRow")) == 1123 and eb.lds_limit(6) == 3370
    assert (kernel_constant("kRcMaxCams"), kernel_constant("kSweepThreads"), eb.DENSE_CAMERAS) == (1100, 1024, 21)


# ---- the references against the fp64 oracle -----------------------------------------------------------------------------
def _oracle_quantities(orc, problem, st):
    """What the fp64 oracle gives for the case: blocks, and with them y, sd in plain float64 numpy."""
    args, x = eb.problem(problem, orc)
    C, P, ci, pi = args[0], args[1], np.asarray(args[2]), np.asarray(args[3])
    lin = eb.linearisation(problem, orc)
    dc, dp, v = eb.operands(lin, st)
    r, Jc, Jp = orc.jacobian_blocks(x, *args)
    nb = orc.normal_blocks(r, Jc, Jp, C, P, ci, pi)
    Vd = nb.V.copy()
    Vd[:, np.arange(3), np.arange(3)] += dp.reshape(P, 3)
    Vinv = np.linalg.inv(Vd)
    vc = v.reshape(C, 6)
    yy = np.zeros((P, 3))
    np.add.at(yy, pi, np.einsum("nij,ni->nj", nb.W, vc[ci]))
    z = np.einsum("pij,pj->pi", Vinv, yy)
    y = np.einsum("cij,cj->ci", nb.U, vc) + dc.reshape(C, 6) * vc
    np.add.at(y, ci, -np.einsum("nij,nj->ni", nb.W, z[pi]))
    sd = np.zeros((C, 6, 6))
    np.add.at(sd, ci, np.einsum("nij,njk,nlk->nil", nb.W, Vinv[pi], nb.W))
    return {"r": r, "Jc": Jc, "Jp": Jp, "U": nb.U, "V": nb.V, "gc": nb.gc, "gp": nb.gp, "y": y, "sd": sd}, (dc, dp, v)


@pytest.mark.parametrize("problem", ["hand_built", "theta_sweep", "schur_1024"])
def test_longdouble_references_agree_with_the_oracle(orc, problem):
    """The oracle is the same arithmetic in float64 (other operation orders, no more operations on a path): it lies within
    the bounds its own roundings are given here."""
    st = eb.structure(problem, orc, {})
    lin = eb.linearisation(problem, orc)
    o, (dc, dp, v) = _oracle_quantities(orc, problem, st)
    b = lin.blocks(st)
    refs = {"r": (lin.r, lin.k_r, lin.ra), "Jc": (lin.Jc, lin.k_jc, lin.Jca), "Jp": (lin.Jp, lin.k_jp, lin.Jpa)}
    for q in ("U", "V", "gc", "gp"):
        refs[q] = (b[q], b["k_" + q], b[q + "a"])
    s = lin.schur_product(st, dc, dp, v, "stored")
    refs["y"] = (s["y"], s["k_y"], s["ya"])
    rp = lin.rhs_pass(st, dc, dp)
    refs["sd"] = (rp["sd"], rp["k_sd"], rp["sda"])
    for q, (ref, k, A) in refs.items():
        assert eb.ratio(o[q].reshape(ref.shape), ref, eb.bound(k, A)) <= 1.0, (problem, q)


# ---- what the per-entry check sees and the normwise check does not ---------------------------------------------------------
def test_fp32_rounding_of_the_smallest_entries_is_rejected_entry_by_entry_and_accepted_normwise(orc):
    """The oracle's values as the "device output", with the smallest hundredth of the non-zero entries of one quantity
    rounded to fp32: the bounds of test_gpu_entries.py reject it, the max-norm figures of test_gpu_parity.py accept it."""
    st = eb.structure("hand_built", orc, {})
    lin = eb.linearisation("hand_built", orc)
    o, (dc, dp, v) = _oracle_quantities(orc, "hand_built", st)
    b = lin.blocks(st)
    s, rp = lin.schur_product(st, dc, dp, v, "rc"), lin.rhs_pass(st, dc, dp)
    cases = {"U": (b["U"], b["k_U"], b["Ua"], 1e-11), "V": (b["V"], b["k_V"], b["Va"], 1e-11), "gc": (b["gc"], b["k_gc"], b["gca"], 1e-10),
             "y": (s["y"], s["k_y"], s["ya"], 1e-9), "sd": (rp["sd"], rp["k_sd"], rp["sda"], 1e-11)}
    for q, (ref, k, A, normwise) in cases.items():
        bnd = eb.bound(k, A)
        clean = o[q].reshape(ref.shape)
        assert eb.ratio(clean, ref, bnd) <= 1.0, q
        mag = np.abs(clean)
        cut = np.quantile(mag[mag > 0], 0.01)
        small = (mag > 0) & (mag <= cut)
        spoilt = np.where(small, clean.astype(np.float32).astype(np.float64), clean)
        assert np.any(spoilt != clean), q
        worst = eb.ratio(spoilt, ref, bnd)
        print(f"{q}: {int(small.sum())} entries rounded to fp32: err/bound {worst:.3g}, normwise {eb.rel_max(spoilt, np.asarray(ref, dtype=np.float64)):.3g}")
        assert worst > 1.0, q                                                          # the per-entry check rejects it
        assert eb.rel_max(spoilt, np.asarray(ref, dtype=np.float64)) < normwise, q     # test_gpu_parity.py's check accepts it


def test_relative_error_the_entry_check_lets_through(orc):
    """How small an error the bounds still see, in units of eps relative to the entry: bound / (eps |ref|), at the best
    and at the median entry of every quantity of the hand-built problem (printed; DESIGN.md section 20 has the figures).
    U and V see 54 .. 69 eps on their best entries and 1.2e3 .. 1.7e3 at the median; the deeper quantities, with both
    factors of every product counted, 1e4 .. 1e5 eps at the median -- 2e-12 .. 2e-11 of the ENTRY, where the max-norm
    check allows 1e-11 of the LARGEST entry.  Asserted: the same relative error of 1e-11 on every entry, which the
    normwise check accepts by construction, is rejected by every quantity."""
    st = eb.structure("hand_built", orc, {})
    lin = eb.linearisation("hand_built", orc)
    dc, dp, v = eb.operands(lin, st)
    b, rp, s = lin.blocks(st), lin.rhs_pass(st, dc, dp), lin.schur_product(st, dc, dp, v, "rc")
    cases = {q: (b[q], b["k_" + q], b[q + "a"]) for q in ("U", "V", "gc", "gp")}
    cases.update({q: (rp[q], rp["k_" + q], rp[q + "a"]) for q in ("rhs", "sd", "minv")})
    cases["y"] = (s["y"], s["k_y"], s["ya"])
    for q, (ref, k, A) in cases.items():
        bnd = eb.bound(k, A)
        nz = ref != 0
        level = np.asarray(bnd[nz] / np.abs(ref[nz]), dtype=np.float64) / eb.EPS
        print(f"{q}: bound / (eps |ref|) best {level.min():.0f}, median {np.median(level):.0f}")
        spoilt = np.asarray(ref, dtype=np.float64) * (1 + 1e-11)
        assert eb.ratio(spoilt, ref, bnd) > 1.0, q
        assert eb.rel_max(spoilt, np.asarray(ref, dtype=np.float64)) <= 1.01e-11, q
