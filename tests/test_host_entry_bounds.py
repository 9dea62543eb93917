"""tests/entry_bounds.py without a GPU: the conditions that keep the bounds of test_gpu_entries.py meaningful hold for
every one of its cases, the longdouble references agree with the fp64 oracle to the oracle's own rounding, and the
per-entry check rejects what the normwise check of test_gpu_parity.py lets through."""
import numpy as np
import pytest

import entry_bounds as eb
import entry_bounds32 as e32

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


# ---- fp32 storage and the mixed-precision product (tests/entry_bounds32.py, test_gpu_entries32.py) -----------------------------
def _host_fetch(orc, name, cases=None):
    """What test_gpu_entries32.py fetches from the device, emulated for a case: the operands rounded from x, V of the
    longdouble blocks as doubles, the blocks of the fp64 oracle at the pixels the storage mode holds."""
    args, x, lin, st, (dc, dp, v), options, forms, bits = e32.case(name, orc, cases)
    ops = e32.operands_from_x(lin, x, v)
    uv = np.asarray(args[4], dtype=np.float64)
    if bits == 32:
        uv = uv.astype(np.float32).astype(np.float64)
    r, Jc, Jp = orc.jacobian_blocks(x, args[0], args[1], args[2], args[3], uv, args[5])
    V = np.asarray(lin.blocks(st)["V"], dtype=np.float64)
    return args, x, lin, st, (dc, dp, v), forms, ops, V, (r, Jc, Jp)


@pytest.mark.parametrize("name", list(e32.MIXED_CASES))
def test_mixed_cases_tie_entries_and_the_fp64_oracle(orc, name):
    """Every array of every mixed case: tie entries within TIE_CAP (none in the emulated a', which is not fetched); the
    same operand roundings followed by plain double arithmetic lie inside every bound, and y meets SHARE / LEVEL_Y."""
    args, x, lin, st, (dc, dp, v), forms, ops, V, (_, _, Jp) = _host_fetch(orc, name)
    assert not ops["a_tie"].any(), name
    rt32 = e32.fl32(ops["rt"])
    ok, tie_rt = e32.accepted32(rt32, ops["rt"], ops["rt_bnd"])
    assert ok.all() and np.array_equal(rt32[:, 9:], ops["T32"]), name
    mixed_b = forms["mixed_b"] == 1
    kw = dict(mixed_b=mixed_b, a32=ops["a32"], uT32=ops["uT32"])
    ref = e32.mixed_product(lin, st, args[5], dc, dp, v, rt32, ops["X32"], V, **kw)
    o64 = e32.mixed_product(lin, st, args[5], dc, dp, v, rt32, ops["X32"], V, dt=np.float64, rows64=Jp, **kw)
    seen, A, B = lin.Lp > 0, ref["a"], ref["b"]
    bz = eb.bound(A["k_z"], A["za"])
    ok, tie_z = e32.accepted32(e32.fl32(o64["a"]["z"])[seen], A["z"][seen], bz[seen])
    assert ok.all(), name
    assert eb.ratio(o64["a"]["z"][seen], A["z"][seen], bz[seen]) <= 1.0, name
    by = eb.bound(B["k_y"], B["ya"])
    q, s = eb.ratio(o64["b"]["y"], B["y"], by), eb.share_below(by, B["y"], eb.LEVEL_Y)
    print(f"{name}: tie share rt32 {tie_rt.mean():.2e}, z32 {tie_z.mean():.2e}; fp64 oracle err/bound of y {q:.3f}, share below "
          f"{eb.LEVEL_Y:g} |ref| {s:.4f} (k_z {A['k_z'].min():.0f}..{A['k_z'].max():.0f}, k_y {B['k_y'].min():.0f}..{B['k_y'].max():.0f})")
    assert tie_rt.mean() <= e32.TIE_CAP and tie_z.mean() <= e32.TIE_CAP, name
    assert q <= 1.0 and s >= eb.SHARE, (name, q, s)


@pytest.mark.parametrize("name", list(eb.K1_CASES))
def test_k1_fp32_stores_tie_entries_and_the_fp64_oracle(orc, name):
    problem, _, _ = eb.K1_CASES[name]
    args, x = eb.problem(problem, orc)
    lin = e32.linearisation32(problem, orc, 32)
    uv32 = np.asarray(args[4], dtype=np.float64).astype(np.float32).astype(np.float64)
    o = dict(zip(("r", "Jc", "Jp"), orc.jacobian_blocks(x, args[0], args[1], args[2], args[3], uv32, args[5])))
    for what, ref, k, A in (("r", lin.r, lin.k_r, lin.ra), ("Jc", lin.Jc, lin.k_jc, lin.Jca), ("Jp", lin.Jp, lin.k_jp, lin.Jpa)):
        ok, tie = e32.accepted32(e32.fl32(o[what].reshape(ref.shape)), ref, eb.bound(k, A))
        print(f"{name}: {what} tie share {tie.mean():.2e} ({int(tie.sum())} of {tie.size})")
        assert ok.all() and tie.mean() <= e32.TIE_CAP, (name, what, tie.mean())


@pytest.mark.parametrize("name", list(eb.RHS_CASES))
def test_rhs_cases_at_the_pixels_of_fp32_storage(orc, name):
    problem, options, _ = eb.RHS_CASES[name]
    lin, st = e32.linearisation32(problem, orc, 32), eb.structure(problem, orc, options)
    dc, dp, _ = eb.operands(lin, st)
    ref = lin.rhs_pass(st, dc, dp)
    _share(name, "rhs", ref["rhs"], ref["k_rhs"], ref["rhsa"])
    _share(name, "sd", eb.upper(ref["sd"]), ref["k_sd"], eb.upper(ref["sda"]))
    _share(name, "minv", eb.upper(ref["minv"]), ref["k_minv"], eb.upper(ref["minva"]), share=eb.SHARE_MINV)


@pytest.mark.parametrize("name", list(e32.STORED_CASES))
def test_stored_fp32_jacobian_cases(orc, name):
    args, x, lin, st, (dc, dp, v), forms, ops, V, (_, Jc, Jp) = _host_fetch(orc, name, e32.STORED_CASES)
    Jc32, Jp32 = Jc.astype(np.float32), Jp.astype(np.float32)
    ref = e32.stored_product(lin, st, Jc32, Jp32, V, dc, dp, v)
    o64 = e32.stored_product(lin, st, Jc32, Jp32, V, dc, dp, v, dt=np.float64)
    by = eb.bound(ref["k_y"], ref["ya"])
    q, s = eb.ratio(o64["y"], ref["y"], by), eb.share_below(by, ref["y"], eb.LEVEL_Y)
    print(f"{name}: fp64 oracle err/bound of y {q:.3f}, share below {eb.LEVEL_Y:g} |ref| {s:.4f}")
    assert q <= 1.0 and s >= eb.SHARE, (name, q, s)


def test_pass_b_in_its_own_form_is_the_schur_product(orc):
    """entry_bounds32.pass_b fed with the fp64 quantities of x is entry_bounds' schur_product: value and abs-value evaluation."""
    st, lin = eb.structure("hand_built", orc, {}), eb.linearisation("hand_built", orc)
    dc, dp, v = eb.operands(lin, st)
    s, pv = lin.schur_product(st, dc, dp, v, "rc"), lin.point_inverses(st, dp)
    vc = v.reshape(lin.C, 6).astype(eb.LD)
    ap, apa, k_ap = lin._a_prime(vc)
    yp = np.zeros((lin.P, 3), dtype=eb.LD)
    np.add.at(yp, lin.pi, np.einsum("nki,nk->ni", lin.Jp, np.einsum("nki,ni->nk", lin.Jc, vc[lin.ci])))
    z = np.einsum("pij,pj->pi", pv["Vinv"], yp)
    B = e32.pass_b(lin, st, lin.Jp, lin.Jps, lin.ka_jp, lin.v, lin.va, 1, ap, apa, k_ap, vc[:, 3:], z, np.abs(z), 0.0, dc, v)
    assert np.abs(np.asarray(B["y"] - s["y"], dtype=np.float64)).max() <= 1e-16 * float(np.abs(s["y"]).max())
    assert np.all(B["k_y"] <= s["k_y"]) and np.all(B["ya"] <= s["ya"] * (1 + 1e-15))


def test_planted_errors_are_rejected_entry_by_entry_and_accepted_by_the_normwise_window(orc):
    """What the 1e-13 < rel < 1e-6 window of test_mixed_precision_schur_product (and the 1e-6 of test_fp32_storage_mode)
    cannot tell from the contract "fp32 operands, fp64 arithmetic", planted into the fp64 oracle's values of the
    hand-built case: each is rejected by the check of test_gpu_entries32.py and accepted by the window it replaces."""
    args, x, lin, st, (dc, dp, v), forms, ops, V, (_, Jc, _) = _host_fetch(orc, "default")
    K, F32 = args[5], np.float32
    rt32 = e32.fl32(ops["rt"])
    exact = eb.linearisation("hand_built", orc).schur_product(st, dc, dp, v, "rc")["y"]       # the old test's reference: fp64, x

    def window(y, ref=exact):
        return 1e-13 < eb.rel_max(np.asarray(y, dtype=np.float64), np.asarray(ref, dtype=np.float64)) < 1e-6

    def product(dt, **kw):
        a = dict(mixed_b=True, a32=ops["a32"], uT32=ops["uT32"], rt32=rt32, dc=dc)
        a.update(kw)
        rt, d = a.pop("rt32"), a.pop("dc")
        return e32.mixed_product(lin, st, K, d, dp, v, rt, ops["X32"], V, dt=dt, **a)

    clean = product(np.float64)
    z32 = e32.fl32(clean["a"]["z"])
    ref = product(eb.LD, z32=z32)
    B = ref["b"]
    by = eb.bound(B["k_y"], B["ya"])
    assert eb.ratio(clean["b"]["y"], B["y"], by) <= 1.0 and window(clean["b"]["y"])
    seen, A = lin.Lp > 0, ref["a"]
    bz = eb.bound(A["k_z"], A["za"])
    assert e32.accepted32(z32[seen], A["z"][seen], bz[seen])[0].all()

    # 1. one product of pass B formed in fp32: s0 += u_k j_0 of one observation
    u, j = clean["b"]["u"], clean["rows"].j
    n = int(np.flatnonzero(lin.ci == int(np.argmax(lin.Lc)))[0])
    c = int(lin.ci[n])
    spoilt = np.array(clean["b"]["y"], dtype=np.float64)
    spoilt[c, 3] -= float(F32(u[n, 0] * j[n, 0, 0])) - u[n, 0] * j[n, 0, 0]
    assert spoilt[c, 3] != clean["b"]["y"][c, 3]
    q = eb.ratio(spoilt, B["y"], by)
    print(f"one fp32 product in pass B: err/bound {q:.3g}")
    assert q > 1.0 and window(spoilt)

    # 2. z rounded twice
    z2 = (z32.astype(np.float64) * (1 + 2.0 ** -24)).astype(F32)
    ok = e32.accepted32(z2[seen], A["z"][seen], bz[seen])[0]
    print(f"z rounded twice: {int((~ok).sum())} of {ok.size} entries of z32 rejected")
    assert not ok.all() and window(product(np.float64, z32=z2)["b"]["y"])

    # 3. T rounded absolutely instead of relative to the origin (the unshifted scene)
    T = x[:6 * lin.C].reshape(lin.C, 6)[:, 3:]
    rt_abs = rt32.copy()
    rt_abs[:, 9:] = (T.astype(F32).astype(np.float64) - ops["origin"]).astype(F32)
    ok = e32.accepted32(rt_abs, ops["rt"], ops["rt_bnd"])[0]
    print(f"T rounded absolutely: {int((~ok).sum())} of {3 * lin.C} entries of T - o rejected")
    assert not ok.all() and window(product(np.float64, rt32=rt_abs)["b"]["y"])

    # 4. the smallest hundredth of the stored Jc entries one ulp32 off
    lin32 = e32.linearisation32("hand_built", orc, 32)
    stored = Jc.astype(F32)
    mag = np.abs(stored)
    small = (mag > 0) & (mag <= np.quantile(mag[mag > 0], 0.01))
    off = np.where(small, np.nextafter(stored, F32(np.inf)), stored)
    bj = eb.bound(lin32.k_jc, lin32.Jca)
    assert e32.accepted32(stored, lin32.Jc, bj)[0].all()
    ok = e32.accepted32(off, lin32.Jc, bj)[0]
    print(f"stored Jc one ulp32 off: {int((~ok).sum())} of {int(small.sum())} perturbed entries rejected")
    assert (~ok).sum() == small.sum() and eb.rel_max(off.astype(np.float64), Jc) < 1e-6

    # 5. one observation of a camera's last chunk dropped -- on a product whose largest entry belongs to ANOTHER camera (one
    # strongly damped camera, as a trust-region step with one poorly scaled camera has it): the window is blind to the rest
    c = int(np.argmax(lin.Lc))
    last = int(np.flatnonzero(lin.ci == c)[-1])
    rows = np.abs(np.asarray(exact, dtype=np.float64)).max(axis=1)
    rows[c] = 0.0
    other = int(np.argmax(rows))
    dcs = np.array(dc, dtype=np.float64).reshape(lin.C, 6)
    dcs[other] *= 1e5
    exact_s = eb.linearisation("hand_built", orc).schur_product(st, dcs.ravel(), dp, v, "rc")["y"]
    full, dropped = product(eb.LD, z32=z32, dc=dcs), product(np.float64, z32=z32, dc=dcs, drop=last)
    Bs = full["b"]
    q = eb.ratio(dropped["b"]["y"], Bs["y"], eb.bound(Bs["k_y"], Bs["ya"]))
    print(f"one observation of camera {c} dropped: err/bound {q:.3g}, normwise "
          f"{eb.rel_max(np.asarray(dropped['b']['y'], dtype=np.float64), np.asarray(exact_s, dtype=np.float64)):.3g}")
    assert q > 1.0 and window(dropped["b"]["y"], exact_s)


def test_origin_replica_arguments():
    """The Python replica of upload_x's origin: the sample's stride, and a non-finite point in the sample gives 0."""
    C, P = 2, 10
    x = np.arange(6 * C + 3 * P, dtype=np.float64)
    pts = x[6 * C:].reshape(P, 3)
    assert np.array_equal(e32.origin_of(x, C, P), np.array([sum(pts[:, k].tolist()) / P for k in range(3)]))
    for bad in (np.inf, -np.inf, np.nan):
        y = x.copy()
        y[6 * C + 3 * 4 + 1] = bad
        assert np.array_equal(e32.origin_of(y, C, P), np.zeros(3))
    P = 2500                                                 # stride 2: the odd points are not read
    x = np.concatenate([np.zeros(6 * C), np.random.default_rng(0).normal(size=3 * P)])
    y = x.copy()
    y[6 * C + 3::6] = np.nan
    o = e32.origin_of(x, C, P)
    assert np.array_equal(e32.origin_of(y, C, P), o) and np.allclose(o, x[6 * C:].reshape(P, 3)[::2].mean(axis=0), atol=1e-14)
    assert np.array_equal(e32.origin_of(np.zeros(6 * C), C, 0), np.zeros(3))


def test_fl32_interval_reports_the_tie_entries():
    one, up = np.float32(1.0), np.nextafter(np.float32(1.0), np.float32(2.0))
    mid = (eb.LD(one) + eb.LD(up)) / 2
    ref = np.array([eb.LD(1.0), mid * (1 - eb.LD(1e-12)), mid * (1 + eb.LD(1e-12)), mid * (1 - eb.LD(1e-9))])
    lo, hi, tie = e32.fl32_interval(ref, np.full(4, 1e-11))
    assert tie.tolist() == [False, True, True, False] and lo.tolist() == [one, one, one, one] and hi.tolist() == [one, up, up, one]
    ok, _ = e32.accepted32(np.array([1.0, float(up), 1.0, float(up)]), ref, np.full(4, 1e-11))
    assert ok.tolist() == [True, True, True, False]
    assert not e32.accepted32(np.array([1.0 + 1e-12]), ref[:1], np.full(1, 1e-11))[0][0]      # not a float32 value


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
