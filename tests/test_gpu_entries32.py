"""fp32 storage and the mixed-precision Schur product entry by entry (tests/entry_bounds32.py has the references, the
counts and the contract): K1's fp32 stores against float32 of the rounded-pixel linearisation, bit for bit outside the
tie entries; the normal-equation blocks of fp32 storage within their fp64 bounds; the fp32 operands of the mixed
product (origin, R | T - o, X - o) against their definition; pass A's z32 and pass B's y, each from the fetched
operands of the layer before it; the product on the stored fp32 Jacobian.  One rank, dense = 0, every case a Backend
of its own.  The normwise tests (test_fp32_storage_mode, test_mixed_precision_schur_product, test_gpu_cfg5.py) stay."""
import numpy as np
import pytest

import entry_bounds as eb
import entry_bounds32 as e32
from test_gpu_entries import _assert_structure, _check

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not eb.extended_precision(), reason="numpy.longdouble is no wider than a double on this machine")]

DEFAULTS = dict(tab_lds=-1, vec_lds=-1, cam_chunk=0, sweep_rc=-1, dense=-1, rhsrec=-1, xcd_chunks=-1, xcd_cam=-1, pcg_mixed=-1,
                pcg_mixed_b=-1)
FORMS = ("mixed", "mixed_b", "sweep_rc", "sweep_rc_g", "xcd_b", "cam_multi", "pcg_fused", "round_blocks")


@pytest.fixture(scope="module")
def orc():
    from oracle import ba_oracle
    return ba_oracle


@pytest.fixture
def opened():
    """opened(options, bits) -> a Backend of its own in that storage mode with these debug options and dense = 0; whatever
    it set is reset, and the handle closed, when the test ends."""
    import sfmba
    made = []

    def open_(options, bits):
        be = sfmba.Backend(0)
        made.append((be, ["dense"] + list(options)))
        be.set_precision(bits)
        be.debug_option("dense", 0)
        for name, value in options.items():
            be.debug_option(name, value)
        return be
    yield open_
    for be, names in made:
        for name in names:
            be.debug_option(name, DEFAULTS[name])
        be.close()


def _forms(be, want, tag):
    got = {name: be.form(name) for name in FORMS}
    assert be.form("dense") == 0, tag
    for name, value in want.items():
        assert be.form(name) == value, (tag, name, got)
    return got


def _check32(tag, what, got, ref, bnd, cap=e32.TIE_CAP):
    """An fp32 store: every entry a float inside fl32_interval(ref, bound) -- float32(ref) itself outside the tie entries."""
    got = np.asarray(got)
    ok, tie = e32.accepted32(got, ref, bnd)
    exact = np.asarray(got, dtype=np.float64).reshape(ref.shape) == e32.fl32(ref).astype(np.float64)
    print(f"{tag}: {what} fp32 store: err / (bound + ulp32 / 2) {e32.ratio32(got, ref, bnd):.3f}, {int(tie.sum())} tie entries of "
          f"{tie.size} (share {tie.mean():.2e}), {int((~exact).sum())} entries differ from float32(ref)")
    assert ok.all(), (tag, what, int((~ok).sum()), np.argwhere(~ok)[:5].tolist())
    assert np.all(exact | tie), (tag, what)
    assert tie.mean() <= cap, (tag, what, tie.mean())


# ---- K1's stores and the blocks in fp32 storage ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(eb.K1_CASES))
def test_k1_fp32_stores(opened, orc, name):
    """r, Jc, Jp as k_resjac<F32> stores them: float32 of the linearisation at float32(uv), which the kernel forms in
    fp64 (bounds and cases of test_k1_residual_and_jacobian)."""
    problem, options, forms = eb.K1_CASES[name]
    args, x = eb.problem(problem, orc)
    be = opened(options, 32)
    be.set_problem(*args)
    _forms(be, dict(forms, round_blocks=0, mixed=1, mixed_b=1), name)
    lin = e32.linearisation32(problem, orc, 32)
    r, Jc, Jp = be.residual_jacobian(x)
    _check32(name, "r", r, lin.r, eb.bound(lin.k_r, lin.ra))
    _check32(name, "Jc", Jc, lin.Jc, eb.bound(lin.k_jc, lin.Jca))
    _check32(name, "Jp", Jp, lin.Jp, eb.bound(lin.k_jp, lin.Jpa))


@pytest.mark.parametrize("name", list(eb.BLOCK_CASES))
def test_fp32_storage_recomputes_the_blocks_in_fp64(opened, orc, name):
    """U, g_c, V, g_p of fp32 storage: sums of blocks recomputed in fp64 from float32(uv), within the fp64 bounds of
    test_normal_equation_blocks."""
    problem, options, forms = eb.BLOCK_CASES[name]
    args, x = eb.problem(problem, orc)
    be = opened(options, 32)
    be.set_problem(*args)
    _forms(be, dict(forms, round_blocks=0, mixed=1), name)
    lin, st = e32.linearisation32(problem, orc, 32), eb.structure(problem, orc, options)
    _assert_structure(name, st, lin, be)
    U, V, gc, gp = be.normal_blocks(x)
    b = lin.blocks(st)
    _check(name, "U", U, eb.upper(b["U"]), b["k_U"], eb.upper(b["Ua"]))
    _check(name, "g_c", gc, b["gc"], b["k_gc"], b["gca"])
    _check(name, "V", V, eb.upper(b["V"]), b["k_V"], eb.upper(b["Va"]))
    _check(name, "g_p", gp, b["gp"], b["k_gp"], b["gpa"])


@pytest.mark.parametrize("name", list(eb.RHS_CASES))
def test_rhs_and_preconditioner_pass_in_fp32_storage(opened, orc, name):
    """sfmba_rhs_precond in fp32 storage with a recomputing pass A: the pass reads nothing rounded but the pixels, so
    rhs, sd and the inverse blocks stay within the fp64 bounds of test_rhs_and_preconditioner_pass at float32(uv)."""
    problem, options, forms = eb.RHS_CASES[name]
    args, x = eb.problem(problem, orc)
    be = opened(options, 32)
    be.set_problem(*args)
    _forms(be, dict(forms, round_blocks=0, mixed=1), name)
    lin, st = e32.linearisation32(problem, orc, 32), eb.structure(problem, orc, options)
    _assert_structure(name, st, lin, be)
    dc, dp, _ = eb.operands(lin, st)
    rhs, sd, minv = be.rhs_precond(x, dc, dp)
    ref = lin.rhs_pass(st, dc, dp)
    _check(name, "rhs", rhs, ref["rhs"], ref["k_rhs"], ref["rhsa"])
    _check(name, "sd", sd, eb.upper(ref["sd"]), ref["k_sd"], eb.upper(ref["sda"]))
    _check(name, "minv", minv, eb.upper(ref["minv"]), ref["k_minv"], eb.upper(ref["minva"]), share=eb.SHARE_MINV)


def test_rhs_precond_refuses_the_stored_fp32_jacobian(opened, orc):
    """round_blocks: the pass rounds its blocks to fp32, which is not what the entry's header states."""
    args, x = eb.problem("hand_built", orc)
    be = opened({"sweep_rc": 0}, 32)
    be.set_problem(*args)
    assert be.form("round_blocks") == 1
    with pytest.raises(ValueError):
        be.rhs_precond(x, np.ones(6 * args[0]), np.ones(3 * args[1]))


# ---- the mixed-precision product -----------------------------------------------------------------------------------------------
def _check_operands(tag, m, ops):
    """The fetched operands against their definition: origin and X - o bit for bit, R | T - o by fl32_interval, rtd the
    doubles of rt32."""
    assert np.array_equal(m["origin"], ops["origin"]), (tag, m["origin"], ops["origin"])
    assert np.array_equal(m["rec32"][:, :3], ops["X32"]), tag
    _check32(tag, "rt32", m["rt32"], ops["rt"], ops["rt_bnd"])
    assert np.array_equal(m["rt32"][:, 9:], ops["T32"]), tag
    assert np.array_equal(m["rtd"], m["rt32"].astype(np.float64)), tag


@pytest.mark.parametrize("name", list(e32.MIXED_CASES))
def test_mixed_product_passes(opened, orc, name):
    """One sfmba_schur_matvec on fp32 operands.  The operands against their definition; pass A's z32 (where pass B reads
    fp32 records) by fl32_interval against the reference formed from the FETCHED rt32, X - o, V and the emulated a', u_T;
    pass B's y within k eps A of the reference formed from the fetched z32 and the same operands -- or, pcg_mixed_b = 0,
    of pass A's unrounded z chained into pass B from x."""
    args, x, lin, st, (dc, dp, v), options, forms, bits = e32.case(name, orc)
    be = opened(options, bits)
    be.set_problem(*args)
    _forms(be, forms, name)
    _assert_structure({"cam_chunk64": "cam_chunk64", "xcd": "xcd", "mixed_b0_xcd": "xcd"}.get(name, ""), st, lin, be)
    _, V, _, _ = be.normal_blocks(x)
    y = be.schur_matvec(x, dc, dp, v)
    m = be.mixed_operands()
    ops = e32.operands_from_x(lin, x, v)
    assert not ops["a_tie"].any(), name
    _check_operands(name, m, ops)
    mixed_b = forms["mixed_b"] == 1
    ref = e32.mixed_product(lin, st, args[5], dc, dp, v, m["rt32"], m["rec32"][:, :3], e32.full3(V), mixed_b=mixed_b,
                            z32=m["rec32"][:, 3:6] if mixed_b else None, a32=ops["a32"], uT32=ops["uT32"])
    if mixed_b:
        seen, A = lin.Lp > 0, ref["a"]                      # (a point nobody sees has no z)
        _check32(name, "z32", m["rec32"][seen, 3:6], A["z"][seen], eb.bound(A["k_z"], A["za"])[seen])
    B = ref["b"]
    _check(name, "y", y, B["y"], B["k_y"], B["ya"], level=eb.LEVEL_Y)
    _print_seen(name, lin, y, B)


def _print_seen(tag, lin, y, B):
    """(the largest ratio of y is usually the camera nobody's observations reach: one rounding of dc v against k = 12)"""
    rows = lin.Lc > 0
    q = eb.ratio(np.asarray(y).reshape(lin.C, 6)[rows], B["y"][rows], eb.bound(B["k_y"], B["ya"])[rows])
    print(f"{tag}: y of the cameras with observations err/bound {q:.2e}")


def test_origin_of_a_sampled_point_set(opened, orc):
    """More than 2048 points: the origin is the mean of every second point, in the order upload_x adds them."""
    problem = "origin_%d" % e32.ORIGIN_POINTS
    args, x = e32.problem32(problem, orc)
    C, P = args[0], args[1]
    assert P // 1024 >= 2
    be = opened({}, 32)
    be.set_problem(*args)
    _forms(be, e32._M, problem)
    be.schur_matvec(x, np.ones(6 * C), np.full(3 * P, 1e3), np.ones(6 * C))
    m = be.mixed_operands()
    o = e32.origin_of(x, C, P)
    assert np.array_equal(m["origin"], o) and not np.array_equal(o, x[6 * C:].reshape(P, 3).mean(axis=0))
    assert np.array_equal(m["rec32"][:, :3], (x[6 * C:].reshape(P, 3) - o).astype(np.float32))
    assert np.array_equal(m["rtd"], m["rt32"].astype(np.float64))
    print(f"{problem}: origin {o.tolist()} over {len(range(0, P, P // 1024))} of {P} points")


# ---- the stored fp32 Jacobian --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(e32.STORED_CASES))
def test_product_on_the_stored_fp32_jacobian(opened, orc, name):
    """round_blocks: pass A applies the stored fp32 blocks and pass B rounds its recomputed ones "alike" -- y within
    k eps A of the product of the J that residual_jacobian fetches, taken as the operand of BOTH passes."""
    args, x, lin, st, (dc, dp, v), options, forms, bits = e32.case(name, orc, e32.STORED_CASES)
    be = opened(options, bits)
    be.set_problem(*args)
    _forms(be, {k: w for k, w in forms.items() if k != "lds_vec"}, name)
    assert be.form("lds_vec") == forms["lds_vec"], name
    _, Jc, Jp = be.residual_jacobian(x)
    _, V, _, _ = be.normal_blocks(x)
    y = be.schur_matvec(x, dc, dp, v)
    ref = e32.stored_product(lin, st, Jc, Jp, e32.full3(V), dc, dp, v)
    _check(name, "y", y, ref["y"], ref["k_y"], ref["ya"], level=eb.LEVEL_Y)
    _print_seen(name, lin, y, ref)
    with pytest.raises(ValueError):
        be.mixed_operands()                                   # (no mixed form on this handle)


# ---- the handle afterwards -------------------------------------------------------------------------------------------------------
def test_mixed_operands_leaves_the_handle_as_it_found_it(opened, orc):
    """A solve after sfmba_get_mixed_operands returns the bits of the solve without the call."""
    args, x, lin, st, (dc, dp, v), options, forms, bits = e32.case("default", orc)
    runs = []
    for call in (False, True):
        be = opened(options, bits)
        be.set_problem(*args)
        be.schur_matvec(x, dc, dp, v)
        if call:
            be.mixed_operands()
        opt = be.default_options()
        opt.max_nfev = 6
        xs, res, fun, grad = be.solve(x, opt)
        runs.append((xs, fun, grad, res.nfev, res.cost, be.pcg_history()))
    a, b = runs
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3:] == b[3:]
