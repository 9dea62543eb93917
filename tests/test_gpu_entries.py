"""The solver kernels entry by entry at their form and loop edges: K1's residual and Jacobian, the blocks of the normal
equations (K1's point half, K3), the rhs + preconditioner pass (sfmba_rhs_precond), the implicit Schur product (pass A
and pass B) and the formed reduced camera matrix, each against its longdouble reference within k eps A of
tests/entry_bounds.py -- k counted from the kernel source, A the abs-value evaluation, nothing taken from the device.
fp64 storage, one rank; dense = 0 except where the dense path is the subject.  The conditions that keep the bounds
meaningful (entry_bounds.SHARE ..) are asserted here and, without a GPU, in test_host_entry_bounds.py."""
import numpy as np
import pytest

import entry_bounds as eb

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not eb.extended_precision(), reason="numpy.longdouble is no wider than a double on this machine")]

DEFAULTS = dict(tab_lds=-1, vec_lds=-1, cam_chunk=0, sweep_rc=-1, dense=-1, rhsrec=-1, xcd_chunks=-1, xcd_cam=-1)


@pytest.fixture(scope="module")
def orc():
    from oracle import ba_oracle
    return ba_oracle


@pytest.fixture
def opened():
    """opened(options, dense=0) -> a Backend of its own with these debug options; whatever it set is reset, and the handle
    closed, when the test ends."""
    import sfmba
    made = []

    def open_(options, dense=0):
        be = sfmba.Backend(0)
        made.append((be, ["dense"] + list(options)))
        be.debug_option("dense", dense)
        for name, value in options.items():
            be.debug_option(name, value)
        return be
    yield open_
    for be, names in made:
        for name in names:
            be.debug_option(name, DEFAULTS[name])
        be.close()


def _setup(opened, orc, problem, options, forms, dense=0):
    args, x = eb.problem(problem, orc)
    be = opened(options, dense)
    be.set_problem(*args)
    if dense == 0:
        assert be.form("dense") == 0
    for name, want in forms.items():
        assert be.form(name) == want, (problem, options, name)
    return be, args, x, eb.linearisation(problem, orc), eb.structure(problem, orc, options)


def _check(tag, what, got, ref, k, A, level=eb.LEVEL, share=eb.SHARE):
    """|got - ref| <= k eps A for every entry (printed as the largest ratio), and the bound below level |ref| for `share` of
    the entries."""
    bnd = eb.bound(k, A)
    got = np.asarray(got).reshape(ref.shape)
    q = eb.ratio(got, ref, bnd)
    s = eb.share_below(bnd, ref, level)
    print(f"{tag}: {what} err/bound {q:.2e} (k = {float(np.min(k)):.0f}..{float(np.max(k)):.0f}), share below {level:g} |ref| {s:.4f}")
    assert np.all(np.isfinite(got)), (tag, what)
    assert q <= 1.0, (tag, what, q)
    assert s >= share, (tag, what, s)


def _assert_structure(name, st, lin, be):
    """What the option set is meant to reach: on the handle (sfmba_get_form), and on the problem what makes the form matter.
    entry_bounds.Structure, which counts the sums, must have decided as the handle did."""
    C = lin.C
    assert (be.form("cam_multi"), be.form("xcd_b"), be.form("xcd_cam")) == (st.cam_multi, st.xcd_b, st.xcd_cam), name
    assert be.form("own_inverse") == st.own_inverse and be.form("round_blocks") == 0, name
    assert be.form("rhsrec") == (name == "rhsrec"), name
    if name == "cam_chunk64":                                 # cam_multi: k_cam_combine and k_cam_prep_schur run
        assert st.cam_multi and not st.own_inverse and np.max(np.ceil(lin.Lc / 64.0)) > 2
    elif name in ("xcd", "xcd_pass_b_only"):                  # the XCD-aware table: padded camera group, empty ranges
        assert st.xcd_b and C % eb.source_constant("kWaveChunkCams") != 0
        ranges = np.minimum(lin.pi * eb.source_constant("kWaveChunkRanges") // lin.P, 7)
        assert any(len(np.unique(ranges[lin.ci == c])) < 8 for c in range(C) if lin.Lc[c] > 0) and np.any(lin.Lc == 0)
        assert st.xcd_cam == (name == "xcd")
    elif name == "chunk_edge":
        assert st.chunk_len == 4096 and sorted(lin.Lc)[1:] == [4096, 4097] and st.cam_multi
    elif name in ("default", "rhsrec"):
        assert not st.cam_multi and st.own_inverse and not st.xcd_b and not st.xcd_cam


def test_hand_built_structure(orc):
    """The loop and tile edges the hand-built problem is there for."""
    from kernel_source import kernel_constant
    lin = eb.linearisation("hand_built", orc)
    rt, ct = eb.source_constant("SFMBA_RHS_THREADS"), kernel_constant("kCamThreads")
    assert (rt, ct, eb.TILE) == (192, 256, 64)
    assert sorted(lin.Lc) == sorted([0, 1, rt - 1, rt, rt + 1, 2 * rt - 1, 2 * rt, 2 * rt + 1, 3 * rt + 1,
                                     ct - 1, ct, ct + 1, 2 * ct - 1, 2 * ct, 2 * ct + 1])
    assert lin.C % eb.source_constant("kWaveChunkCams") != 0 and lin.N < 9000
    assert {1, 63, 64, 65, 128, 256, 300} <= set(lin.Lp) and np.any(lin.Lp == 0)
    start = np.concatenate([[0], np.cumsum(lin.Lp)])[:-1]
    end = start + lin.Lp
    seen = lin.Lp > 0
    assert np.any(seen & (lin.Lp < 64) & (end % 64 == 0)) and np.any(seen & (start % 64 == 0) & (start > 0) & (lin.Lp % 64 != 0))
    assert np.any((end // 64) - ((start + 63) // 64) >= 2)      # two whole tiles inside one run: point_edge_fixup adds rows


@pytest.mark.parametrize("name", list(eb.K1_CASES))
def test_k1_residual_and_jacobian(opened, orc, name):
    """r, Jc, Jp of k_resjac with the camera table in LDS and read through the LDS-DMA slabs (tab_lds = 0; one camera more
    than the LDS takes), on the hand-built runs and on the small-angle fixture."""
    problem, options, forms = eb.K1_CASES[name]
    be, args, x, lin, _ = _setup(opened, orc, problem, options, forms)
    r, Jc, Jp = be.residual_jacobian(x)
    _check(name, "r", r, lin.r, lin.k_r, lin.ra)
    _check(name, "Jc", Jc, lin.Jc, lin.k_jc, lin.Jca)
    _check(name, "Jp", Jp, lin.Jp, lin.k_jp, lin.Jpa)


@pytest.mark.parametrize("name", list(eb.BLOCK_CASES))
def test_normal_equation_blocks(opened, orc, name):
    """U, g_c (k_cam_blocks, k_cam_combine; k_cam_blocks_w, k_cam_combine_w) and V, g_p (k_resjac's run sums and
    point_edge_fixup)."""
    problem, options, forms = eb.BLOCK_CASES[name]
    be, args, x, lin, st = _setup(opened, orc, problem, options, forms)
    _assert_structure(name, st, lin, be)
    U, V, gc, gp = be.normal_blocks(x)
    b = lin.blocks(st)
    _check(name, "U", U, eb.upper(b["U"]), b["k_U"], eb.upper(b["Ua"]))
    _check(name, "g_c", gc, b["gc"], b["k_gc"], b["gca"])
    _check(name, "V", V, eb.upper(b["V"]), b["k_V"], eb.upper(b["Va"]))
    _check(name, "g_p", gp, b["gp"], b["k_gp"], b["gpa"])


@pytest.mark.parametrize("name", list(eb.RHS_CASES))
def test_rhs_and_preconditioner_pass(opened, orc, name):
    """sfmba_rhs_precond: the reduced right-hand-side term, the Schur-diagonal blocks and the inverse preconditioner blocks
    of k_cam_rhs_diag with its own inverse, with k_cam_combine + k_cam_prep_schur, from the 128-byte records, and of
    k_cam_rhs_diag_w + k_cam_combine_w.  The inverse is spd6_inverse's in every form (entry_bounds.SPD6_ROUNDINGS)."""
    problem, options, forms = eb.RHS_CASES[name]
    be, args, x, lin, st = _setup(opened, orc, problem, options, forms)
    _assert_structure(name, st, lin, be)
    dc, dp, _ = eb.operands(lin, st)
    rhs, sd, minv = be.rhs_precond(x, dc, dp)
    ref = lin.rhs_pass(st, dc, dp)
    _check(name, "rhs", rhs, ref["rhs"], ref["k_rhs"], ref["rhsa"])
    _check(name, "sd", sd, eb.upper(ref["sd"]), ref["k_sd"], eb.upper(ref["sda"]))
    _check(name, "minv", minv, eb.upper(ref["minv"]), ref["k_minv"], eb.upper(ref["minva"]), share=eb.SHARE_MINV)


def test_rhs_precond_leaves_the_handle_as_it_found_it(opened, orc):
    """A solve after sfmba_rhs_precond returns the bits of the solve without the call."""
    args, x = eb.problem("hand_built", orc)
    runs = []
    for call in (False, True):
        be = opened({})
        be.set_problem(*args)
        if call:
            lin, st = eb.linearisation("hand_built", orc), eb.structure("hand_built", orc, {})
            dc, dp, _ = eb.operands(lin, st)
            be.rhs_precond(x, dc, dp)
        opt = be.default_options()
        opt.max_nfev = 6
        xs, res, fun, grad = be.solve(x, opt)
        runs.append((xs, fun, grad, res.nfev, res.cost, be.pcg_history()))
    a, b = runs
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3:] == b[3:]


@pytest.mark.parametrize("name", list(eb.SCHUR_CASES))
def test_schur_product(opened, orc, name):
    """y = S v of sfmba_schur_matvec: pass A recomputing from the LDS table, from the table in global memory, reading the
    stored Jacobian with the vector in LDS and gathered from L2; pass B over the chunk list, with several chunks per camera
    and over the XCD-aware table; the default form either side of 1024, kRcMaxCams and the last vector the LDS takes."""
    problem, options, forms, pass_a = eb.SCHUR_CASES[name]
    be, args, x, lin, st = _setup(opened, orc, problem, options, forms)
    _assert_structure(name, st, lin, be)
    dc, dp, v = eb.operands(lin, st)
    y = be.schur_matvec(x, dc, dp, v)
    ref = lin.schur_product(st, dc, dp, v, pass_a)
    _check(name, "y", y, ref["y"], ref["k_y"], ref["ya"], level=eb.LEVEL_Y)


def test_dense_reduced_camera_matrix(opened, orc):
    """Every entry of the S that k_schur_blocks forms at the last camera count of the dense path."""
    problem = "dense_%d" % eb.DENSE_CAMERAS
    be, args, x, lin, st = _setup(opened, orc, problem, {}, {"dense": 1}, dense=-1)
    dc, dp, v = eb.operands(lin, st)
    S, _ = be.dense_schur(x, dc, dp, v)
    ref = lin.dense_s(st, dc, dp)
    _check(problem, "S", S, ref["S"], ref["k_S"], ref["Sa"], level=eb.LEVEL_Y)


def test_first_camera_count_past_the_dense_path(opened, orc):
    """One camera more: the dense path is off and a whole solve follows the oracle with the implicit settings."""
    from test_gpu_parity import _oracle_kwargs
    args, x = eb.problem("dense_%d" % (eb.DENSE_CAMERAS + 1), orc)
    be = opened({}, dense=-1)
    be.set_problem(*args)
    assert be.form("dense") == 0
    opt = be.default_options()
    opt.ftol = 1e-10
    _, res, _, _ = be.solve(x, opt)
    o = orc.trf_schur(x, *args, ftol=1e-10, **_oracle_kwargs(False))
    assert (res.status, res.nfev, res.njev) == (o.status, o.nfev, o.njev)
    assert abs(res.cost - o.cost) <= 1e-9 * o.cost
