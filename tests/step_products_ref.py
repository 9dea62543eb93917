"""sfmba_step_products (k_jdot, k_backsub) entry by entry: the longdouble references, the per-entry bounds, the cases of
tests/test_gpu_step_products.py and tests/test_host_step_products.py, and an emulation of the two kernels in plain float64
numpy that stands in for a Backend where there is no device.  _Case and _check_entries came from
tests/test_gpu_rc_consumers.py, whose header has the counts of the 64-bit fetched-operand form; they are unchanged for it.

The operands of a case (`operands`, with the storage `bits`)
  "fetched", 64   the reference is formed from the blocks be.residual_jacobian FETCHES.  They carry K1's roundings of the same
                  paths, so k is TWICE the kernel's count (the header of test_gpu_rc_consumers.py).
  "fetched", 32   fp32 storage, stored-Jacobian readers.  Taken as EXACT: Jc, Jp as be.residual_jacobian fetches them (the
                  stored float32 values load_blocks reads), V and g_p as be.normal_blocks fetches them (k_point_prep and
                  solve_point read these very doubles) and, for G12, the fetched t1 (the float32 values load_pair reads back).
                  tests/test_gpu_entries32.py holds those layers to their own bounds; a layer is checked from the fetched
                  output of the layer before it.
  "x", 64 or 32   the J-free iteration: K1 stores no blocks, the kernels recompute them by observe<> from the camera table.
                  The reference takes them from entry_bounds.Linearisation at x with the counts k_jc, k_jp and abs-value
                  evaluations Jca, Jpa that test_gpu_entries.py checks K1's Jc and Jp with; V and g_p fetched, exact.
The counts of the exact-operand forms, from the kernel text (k_jdot, k_backsub<..>: jcv, solve_point, gram), every
multiplication and addition one rounding.  An exact operand carries no rounding, so NOTHING is doubled: the count is the
kernel's own, plus the operand's count k_j where the operand is computed (J-free), both factors of a product counted
(k_a + k_b + 1, entry_bounds._mul: rigorous to first order with the nested abs-value evaluations):
    t1 = nine products added to 0:  max(k_jc, k_jp) + T1_ROUNDINGS[0] = k_j + 10
    t = jc . u, six products added to 0:  k_jc + T_ROUNDINGS[0] = k_jc + 7
    y_p = sum of jp^T t:  a product k_jp + k_t + 1, the row pair's addition 1, then the run (_run_roundings)
    dp = Vinv (-g_p - y):  the subtraction 1, three products and two additions 3: k_y + 4 on |Vinv| (|g_p| + A(y));
         Vinv by chol3_inverse from the fetched V + diag: 1 + CHOL_ROUNDINGS on |Vinv| |V + diag| |Vinv| |b|
    t2 = t + jp . dp:  max(k_t, k_jp) + 4 on A(t) + A(jp) |dp|, and A(jp) B(dp)
    sums:  products 2, the lane's windows, wave_sum 6, the workgroup's waves 16, the partial rows -- n_add of _Case.sums, ONCE.
fp32 storage rounds exactly one value of these kernels: store_pair's float32(t1).  k_jdot sums G11 from the UNROUNDED t1
(its reference: the sum of the longdouble t1^2); k_backsub reads the stored t1 back for G12 (its reference: the fetched t1
times the longdouble t2).  The stored t1 is checked with entry_bounds32.fl32_interval: float32(reference) except at tie entries."""
import math

import numpy as np

import entry_bounds as eb
import entry_bounds32 as e32
from entry_bounds import CHOL_ROUNDINGS, EPS, LD, T1_ROUNDINGS, T_ROUNDINGS, _inv3, _row_form_abs, _run_roundings

F32 = np.float32


class _Case:
    """Reference values of sfmba_step_products in longdouble, and what bounds the entries' errors (the module's header:
    `operands`, `bits`; lin: the entry_bounds.Linearisation at pb.x0 of operands "x")."""

    def __init__(self, be, pb, seed=0, operands="fetched", bits=64, lin=None):
        C, P, N = pb.n_cameras, pb.n_points, len(pb.camera_indices)
        ci, pi = np.asarray(pb.camera_indices), np.asarray(pb.point_indices)
        rng = np.random.default_rng(seed)
        self.pb, self.C, self.P, self.N, self.ci, self.pi = pb, C, P, N, ci, pi
        self.operands, self.bits = operands, bits
        self.doubled = operands == "fetched" and bits == 64
        self.sg = rng.normal(size=6 * C + 3 * P)
        self.dc = 1e-2 * rng.normal(size=6 * C)
        self.L = np.bincount(pi, minlength=P)
        self.seen = self.L > 0
        if self.doubled:
            self._from_fetched_fp64_blocks(be, rng)
        else:
            self._from_exact_operands(be, rng, lin)

    def _from_fetched_fp64_blocks(self, be, rng):
        pb, C, P, N, ci, pi = self.pb, self.C, self.P, self.N, self.ci, self.pi
        r, Jc, Jp = be.residual_jacobian(pb.x0)
        r, Jc, Jp = r.reshape(N, 2).astype(LD), Jc.astype(LD), Jp.astype(LD)
        V = np.zeros((P, 3, 3), dtype=LD)
        np.add.at(V, pi, np.einsum("nki,nkj->nij", Jp, Jp))
        # a diagonal of the size of V's own: V + diag is well conditioned, also for a point with one observation (V singular)
        self.diag = np.asarray(np.einsum("pii->pi", V) + 1.0, dtype=np.float64).ravel() * rng.uniform(0.5, 2.0, size=3 * P)
        sgc, sgp, dc = self.sg[:6 * C].reshape(C, 6).astype(LD), self.sg[6 * C:].reshape(P, 3).astype(LD), self.dc.reshape(C, 6).astype(LD)
        aJc, aJp = np.abs(Jc), np.abs(Jp)
        self.t1 = np.einsum("nki,ni->nk", Jc, sgc[ci]) + np.einsum("nki,ni->nk", Jp, sgp[pi])
        t = np.einsum("nki,ni->nk", Jc, dc[ci])
        ja1, ta1 = _row_form_abs(pb, pb.x0, sgc)
        ja2, ta2 = _row_form_abs(pb, pb.x0, dc)
        # sum |terms| of t1 and of t = Jc dc, per form
        self.S_t1 = {0: np.einsum("nki,ni->nk", aJc, np.abs(sgc[ci])) + np.einsum("nki,ni->nk", aJp, np.abs(sgp[pi])),
                     1: ta1 + np.einsum("nki,ni->nk", ja1, np.abs(sgp[pi]))}
        S_t = {0: np.einsum("nki,ni->nk", aJc, np.abs(dc[ci])), 1: ta2}
        aj = {0: aJp, 1: ja2}
        gp, y = np.zeros((P, 3), dtype=LD), np.zeros((P, 3), dtype=LD)
        np.add.at(gp, pi, np.einsum("nki,nk->ni", Jp, r))
        np.add.at(y, pi, np.einsum("nki,nk->ni", Jp, t))
        A = V + np.einsum("pi,ij->pij", self.diag.reshape(P, 3).astype(LD), np.eye(3, dtype=LD))
        Ainv = _inv3(A)
        self.dp = np.einsum("pij,pj->pi", Ainv, -gp - y)
        aInv = np.abs(Ainv)
        ga, aA = np.zeros((P, 3), dtype=LD), np.abs(A)
        np.add.at(ga, pi, np.einsum("nki,nk->ni", aJp, np.abs(r)))
        s_run = _run_roundings(self.L)
        self.k_t1, self.B_t1, self.S_dp, self.k_dp, self.B_dp, self.B_t2 = {}, {}, {}, {}, {}, {}
        self.t2 = t + np.einsum("nki,ni->nk", Jp, self.dp[pi])
        for form in (0, 1):
            self.k_t1[form] = 2 * T1_ROUNDINGS[form]
            self.B_t1[form] = self.k_t1[form] * EPS * self.S_t1[form]
            ya = np.zeros((P, 3), dtype=LD)
            np.add.at(ya, pi, np.einsum("nki,nk->ni", aj[form], S_t[form]))
            # sum |terms| of dp: |Vinv| (sum |jp r| + sum |jp t|), and the inverse's own error |Vinv| |V + diag| |Vinv| |b|
            self.S_dp[form] = np.einsum("pij,pj->pi", aInv, ga + ya) + \
                np.einsum("pij,pjk,pkl,pl->pi", aInv, aA, aInv, np.abs(gp) + np.abs(y))
            self.k_dp[form] = 2 * (T_ROUNDINGS[form] + 2 + s_run + 4 + CHOL_ROUNDINGS + 2 + s_run)
            self.B_dp[form] = self.k_dp[form][:, None] * EPS * self.S_dp[form]
            self.B_t2[form] = 2 * (T_ROUNDINGS[form] + 4) * EPS * (S_t[form] + np.einsum("nki,ni->nk", aj[form], np.abs(self.dp[pi]))) + \
                np.einsum("nki,ni->nk", aj[form], self.B_dp[form][pi])

    def _from_exact_operands(self, be, rng, lin):
        """fp32 stored blocks, or the J-free blocks from x: the module's header has the counts.  Form 0 only (fp32 storage
        and the J-free iteration never run the row form)."""
        pb, C, P, N, ci, pi = self.pb, self.C, self.P, self.N, self.ci, self.pi
        _, V6, _, gp = be.normal_blocks(pb.x0)
        V, gp = e32.full3(np.asarray(V6, dtype=np.float64)).astype(LD), np.asarray(gp, dtype=np.float64).reshape(P, 3).astype(LD)
        if self.operands == "fetched":
            _, Jc, Jp = be.residual_jacobian(pb.x0)
            assert np.array_equal(Jc.astype(F32), Jc) and np.array_equal(Jp.astype(F32), Jp), "fp32 storage fetches float32 values"
            Jc, Jp = Jc.astype(LD), Jp.astype(LD)
            Jca, Jpa, k_jc, k_jp = np.abs(Jc), np.abs(Jp), np.zeros(N), np.zeros(N)
        else:
            Jc, Jp, Jca, Jpa = lin.Jc, lin.Jp, lin.Jca, lin.Jpa
            k_jc, k_jp = np.asarray(lin.k_jc, dtype=np.float64), np.asarray(lin.k_jp, dtype=np.float64)
        self.diag = np.asarray(np.einsum("pii->pi", V) + 1.0, dtype=np.float64).ravel() * rng.uniform(0.5, 2.0, size=3 * P)
        sgc, sgp, dc = self.sg[:6 * C].reshape(C, 6).astype(LD), self.sg[6 * C:].reshape(P, 3).astype(LD), self.dc.reshape(C, 6).astype(LD)
        self.t1 = np.einsum("nki,ni->nk", Jc, sgc[ci]) + np.einsum("nki,ni->nk", Jp, sgp[pi])
        t = np.einsum("nki,ni->nk", Jc, dc[ci])
        self.S_t1 = {0: np.einsum("nki,ni->nk", Jca, np.abs(sgc[ci])) + np.einsum("nki,ni->nk", Jpa, np.abs(sgp[pi]))}
        k_t1 = np.maximum(k_jc, k_jp) + T1_ROUNDINGS[0]
        self.k_t1, self.B_t1 = {0: int(k_t1.max())}, {0: k_t1[:, None] * EPS * self.S_t1[0]}
        S_t, k_t = np.einsum("nki,ni->nk", Jca, np.abs(dc[ci])), k_jc + T_ROUNDINGS[0]
        y, ya = np.zeros((P, 3), dtype=LD), np.zeros((P, 3), dtype=LD)
        np.add.at(y, pi, np.einsum("nki,nk->ni", Jp, t))
        np.add.at(ya, pi, np.einsum("nki,nk->ni", Jpa, S_t))
        k_y = eb._group_max(k_jp + k_t + 2, pi, P) + _run_roundings(self.L)
        A = V + np.einsum("pi,ij->pij", self.diag.reshape(P, 3).astype(LD), np.eye(3, dtype=LD))
        Ainv = _inv3(A)
        aInv = np.abs(Ainv)
        self.dp = np.einsum("pij,pj->pi", Ainv, -gp - y)
        self.S_dp = {0: np.einsum("pij,pj->pi", aInv, np.abs(gp) + ya) +
                     np.einsum("pij,pjk,pkl,pl->pi", aInv, np.abs(A), aInv, np.abs(gp) + np.abs(y))}
        self.k_dp = {0: k_y + 4 + CHOL_ROUNDINGS + 1}
        self.B_dp = {0: self.k_dp[0][:, None] * EPS * self.S_dp[0]}
        self.t2 = t + np.einsum("nki,ni->nk", Jp, self.dp[pi])
        self.B_t2 = {0: (np.maximum(k_t, k_jp) + 4)[:, None] * EPS * (S_t + np.einsum("nki,ni->nk", Jpa, np.abs(self.dp[pi]))) +
                     np.einsum("nki,ni->nk", Jpa, self.B_dp[0][pi])}

    def sums(self, out, form):
        """-> (reference of g11 and the ten sums, their bounds) with the gradient and the scale the device formed them with
        -- and, in fp32 storage, the stored t1 it formed G12 with."""
        C, P, N = self.C, self.P, self.N
        g, si = out["g"].astype(LD), out["si"].astype(LD)
        gpt, spt = g[6 * C:].reshape(P, 3)[self.seen], si[6 * C:].reshape(P, 3)[self.seen]
        dp, Bdp = self.dp[self.seen], self.B_dp[form][self.seen]
        dc, gc, sc, sgc = self.dc.astype(LD), g[:6 * C], si[:6 * C], self.sg[:6 * C].astype(LD)
        # additions on the way of a sum: one per window of a lane's range (ranges are cut at max(64, N / 4096) observations,
        # a window completes at least one run), the run trips of the longest point, 6 + 16 in the workgroup, <= 256 partial rows
        n_add = 2 + max(64, math.ceil(N / 4096)) + math.ceil(self.L.max() / 64) + 6 + 16 + min(256, math.ceil(N / 1024))
        t1, t2, B1, B2 = self.t1, self.t2, self.B_t1[form], self.B_t2[form]
        # G12's first factor: the device's own t1 within B1 of the reference, or (fp32 storage) the stored values it read back
        t1s, B1s = (np.asarray(out["t1"], dtype=np.float64).astype(LD), np.zeros_like(B1)) if self.bits == 32 else (t1, B1)
        ref = [np.sum(t1 * t1), np.sum(t1s * t2), np.sum(t2 * t2),
               np.sum(gpt * dp), np.sum((dp * spt) ** 2), np.sum(gpt / spt ** 2 * dp), np.sum(dp * dp),
               np.sum(gc * dc), np.sum((dc * sc) ** 2), np.sum(sgc * dc), np.sum(dc * dc)]
        e = (2 if self.doubled else 1) * n_add * EPS
        bound = [np.sum((2 * np.abs(t1) + B1) * B1) + e * np.sum(t1 * t1),
                 np.sum(B1s * np.abs(t2) + np.abs(t1s) * B2 + B1s * B2) + e * np.sum(np.abs(t1s * t2)),
                 np.sum((2 * np.abs(t2) + B2) * B2) + e * np.sum(t2 * t2),
                 np.sum(np.abs(gpt) * Bdp) + e * np.sum(np.abs(gpt * dp)),
                 np.sum(spt ** 2 * (2 * np.abs(dp) + Bdp) * Bdp) + (e + 4 * EPS) * np.sum((dp * spt) ** 2),
                 np.sum(np.abs(gpt) / spt ** 2 * Bdp) + (e + 6 * EPS) * np.sum(np.abs(gpt / spt ** 2 * dp)),
                 np.sum((2 * np.abs(dp) + Bdp) * Bdp) + e * np.sum(dp * dp),
                 e * np.sum(np.abs(gc * dc)), (e + 4 * EPS) * np.sum((dc * sc) ** 2), e * np.sum(np.abs(sgc * dc)), e * np.sum(dc * dc)]
        return np.array(ref, dtype=LD), np.array(bound, dtype=LD)


SUM_NAMES = ("G11", "G12", "G22", "q5 points", "q6 points", "q7 points", "q8 points", "q5 cameras", "q6 cameras", "q7 cameras",
             "q8 cameras")


def judge(out, form, case):
    """The named checks of one sfmba_step_products result -> dict name -> bool ("t1", "t1 ties" (fp32 storage), "dp",
    the eleven SUM_NAMES, "finite"), and the printed figures."""
    seen = case.seen
    ref, bound = case.sums(out, form)
    got = np.concatenate([[out["g11"]], out["sums"]]).astype(LD)
    err_s = np.abs(got - ref)
    err_dp = np.abs(out["dp"].astype(LD) - case.dp)[seen]
    ok = {"finite": bool(np.all(np.isfinite(out["t1"])) and np.all(np.isfinite(out["dp"][seen])) and
                         np.all(np.isfinite(got.astype(np.float64))))}
    if case.bits == 32:
        acc, tie = e32.accepted32(out["t1"], case.t1, case.B_t1[form])
        exact = np.asarray(out["t1"], dtype=np.float64) == e32.fl32(case.t1).astype(np.float64)
        ok["t1"] = bool(acc.all() and np.all(exact | tie))
        ok["t1 ties"] = bool(tie.mean() <= e32.TIE_CAP)
        fig = (f"t1 fp32 store err / (bound + ulp32 / 2) {e32.ratio32(out['t1'], case.t1, case.B_t1[form]):.3f} "
               f"(k = {case.k_t1[form]}, {int(tie.sum())} tie entries of {tie.size}, {int((~exact).sum())} differ from float32(ref))")
    else:
        err_t1 = np.abs(out["t1"].astype(LD) - case.t1)
        ok["t1"] = bool(np.all(err_t1 <= case.B_t1[form]))
        fig = f"t1 err/bound {float((err_t1 / case.B_t1[form]).max()):.3f} (k = {case.k_t1[form]})"
    ok["dp"] = bool(np.all(err_dp <= case.B_dp[form][seen]))
    for k, name in enumerate(SUM_NAMES):
        ok[name] = bool(err_s[k] <= bound[k])
    fig += (f", dp {float((err_dp / case.B_dp[form][seen]).max()):.3f} (k = {int(case.k_dp[form].min())}..{int(case.k_dp[form].max())}), "
            f"sums {np.array2string(np.asarray(err_s / bound, dtype=np.float64), precision=3)}")
    return ok, fig, (ref, bound, err_s)


def conditions(case, form, ref, bound):
    """The bounds mean something (SHARE and LEVEL of entry_bounds.py): they sit nine digits below all but a hundredth of
    the entries, and below every sum."""
    seen = case.seen
    return {"t1": float(np.mean(case.B_t1[form] < eb.LEVEL * np.abs(case.t1))) >= eb.SHARE,
            "dp": float(np.mean(case.B_dp[form][seen] < eb.LEVEL * np.abs(case.dp[seen]))) >= eb.SHARE,
            "sums": bool(np.all(bound < eb.LEVEL * np.abs(ref)))}


def _check_entries(be, pb, form, case, tag):
    out = be.step_products(pb.x0, case.sg, case.dc, case.diag)
    # (an unobserved point has no run: nothing produces its dp)
    ok, fig, (ref, bound, err_s) = judge(out, form, case)
    print(f"{tag} form {form}: {fig}")
    assert ok["finite"], tag
    assert ok["t1"], tag
    assert ok.get("t1 ties", True), tag
    assert ok["dp"], tag
    assert np.all(err_s <= bound), (tag, err_s / bound)
    # the bounds mean something: they sit nine digits below all but a hundredth of the entries (and all of the sums)
    cond = conditions(case, form, ref, bound)
    assert cond["t1"], tag
    assert cond["dp"], tag
    assert cond["sums"], tag
    return out


# ---- the problems -------------------------------------------------------------------------------------------------------------
def rc_hand_built(orc):
    """8 cameras, 40 points: 21 points of 3 observations (0..62), a run of 5 that starts on lane 63 of the first window, a
    point with 200 observations (more than a window: the long-run path), 8 points with one observation, 9 with four."""
    import sfmba
    from sfmba.synthetic import BAProblem
    base = sfmba.make_problem(8, 40, 400, seed=4)
    counts = [3] * 21 + [5] + [200] + [1] * 8 + [4] * 9
    pi = np.repeat(np.arange(40), counts)
    ci = (np.arange(len(pi)) * 3 + pi) % 8
    args = (8, 40, ci, pi, np.zeros((len(pi), 2)), base.K)
    rng = np.random.default_rng(7)
    uv = orc.compute_residuals(base.x_true, *args).reshape(-1, 2) + rng.normal(0.0, 0.5, (len(pi), 2))
    return BAProblem(8, 40, ci, pi, uv, base.K, base.x0, base.x_true)


VEC = eb.lds_limit(6)                                        # 3370: the last camera count whose vector fits the LDS
_PROBLEMS = {}


def problem(name, orc):
    """The named problem (built once per process) -> a BAProblem."""
    if name not in _PROBLEMS:
        import sfmba
        from sfmba.synthetic import BAProblem
        if name == "rc_hand_built":
            pb = rc_hand_built(orc)
        elif name == "tiny":
            pb = sfmba.make_problem(6, 80, 500, seed=5)
        elif name == "gaps":
            pb = sfmba.drop_observations(sfmba.make_problem(6, 80, 500, seed=5), cameras=(3,), points=(7,))
        else:                                                # hand_built, schur_<cameras> of entry_bounds.py
            args, x = eb.problem(name, orc)
            pb = BAProblem(args[0], args[1], np.asarray(args[2]), np.asarray(args[3]), np.asarray(args[4]), args[5], x, x)
        _PROBLEMS[name] = pb
    return _PROBLEMS[name]


def linearisation(name, orc, bits):
    """The Linearisation of a problem at its x0 as the storage mode sees its pixels (the blocks do not depend on them)."""
    key = ("step lin", name, bits)
    if key not in eb._CACHE:
        pb = problem(name, orc)
        uv = np.asarray(pb.points_2d, dtype=np.float64)
        if bits == 32:
            uv = uv.astype(F32).astype(np.float64)
        eb._CACHE[key] = eb.Linearisation(pb.n_cameras, pb.n_points, pb.camera_indices, pb.point_indices, uv, pb.K, pb.x0)
    return eb._CACHE[key]


def _c(problem_, bits, options, lds_vec, jfree=0, fixed=(), operands="fetched"):
    return dict(problem=problem_, bits=bits, options=options, fixed=fixed, operands=operands,
                forms=dict(lds_vec=lds_vec, jfree=jfree, rc_cons=0))


# name -> problem, storage bits, debug options, held cameras, operands, the forms form() must report
CASES = {}
for _p in ("hand_built", "rc_hand_built", "tiny", "gaps"):
    CASES["64_l2vec_" + _p] = _c(_p, 64, {"vec_lds": 0}, 0)
CASES["64_l2vec_held_camera"] = _c("tiny", 64, {"vec_lds": 0}, 0, fixed=(2,))
CASES["64_last_lds_vec"] = _c("schur_%d" % VEC, 64, {}, 1)
CASES["64_first_l2_vec"] = _c("schur_%d" % (VEC + 1), 64, {}, 0)
for _p in ("hand_built", "rc_hand_built", "tiny"):
    CASES["64_jfree_" + _p] = _c(_p, 64, {"jfree": 1}, 1, jfree=1, operands="x")
for _p in ("hand_built", "rc_hand_built"):
    CASES["32_stored_" + _p] = _c(_p, 32, {"sweep_rc": 0}, 1)
    CASES["32_stored_l2vec_" + _p] = _c(_p, 32, {"sweep_rc": 0, "vec_lds": 0}, 0)
    CASES["32_default_" + _p] = _c(_p, 32, {}, 1)
CASES["32_last_lds_vec"] = _c("schur_%d" % VEC, 32, {}, 1)
CASES["32_first_l2_vec"] = _c("schur_%d" % (VEC + 1), 32, {}, 0)
CASES["32_jfree_hand_built"] = _c("hand_built", 32, {"jfree": 1}, 1, jfree=1, operands="x")
# the J-free form and the stored form it promises the bits of ("same function, same bits", ba_kernels.hpp)
JFREE_TWINS = {"64_jfree_" + _p: "64_l2vec_" + _p for _p in ("hand_built", "rc_hand_built", "tiny")}


def build_case(name, be, orc):
    """-> (pb, _Case) of CASES[name] on the Backend (or Emulation) `be`, which has the problem set."""
    c = CASES[name]
    pb = problem(c["problem"], orc)
    lin = linearisation(c["problem"], orc, c["bits"]) if c["operands"] == "x" else None
    return pb, _Case(be, pb, operands=c["operands"], bits=c["bits"], lin=lin)


# ---- the two kernels in float64 numpy ---------------------------------------------------------------------------------------------
N_CU = 256                                                   # an MI355X
WAVES = eb.kernel_constant("kSweepThreads") // 64            # waves of a sweep workgroup (kWavesPerSweepBlock)
PLANTS = ("g11_from_stored_t1", "g12_from_unrounded_t1", "t_in_fp32", "long_run_tail_dropped", "camera_slice_one_trip",
          "plane_major_dc")


def _wave_sum(x):
    """wave_sum over the last axis (64): four steps inside the rows of 16, then the four row totals in order."""
    x = np.array(x, dtype=np.float64).reshape(x.shape[:-1] + (4, 16))
    for s in (8, 4, 2, 1):
        x = x[..., :s] + x[..., s:2 * s]
    x = x[..., 0]
    return ((x[..., 0] + x[..., 1]) + x[..., 2]) + x[..., 3]


def _seg_reduce(v, key):
    """seg_reduce_serial on (64, n) values with sorted keys: the first lane of a run of equal keys ends with the run's sum."""
    lane = np.arange(64)
    col, row = lane & 15, lane >> 4
    x = np.array(v, dtype=np.float64)
    for n in (1, 2, 4, 8):
        src = np.minimum(lane + n, 63)
        m = (col + n < 16) & (key[src] == key)
        x = x + np.where(m[:, None], x[src], 0.0)
    for r, f in ((2, 48), (1, 32), (0, 16)):
        m = (row == r) & (key == key[f])
        x = x + np.where(m[:, None], x[f][None, :], 0.0)
    return x


def _chol3_inverse(a):
    """chol3_inverse of ba_device.hpp on (P, 6) packed upper triangles, operation by operation."""
    a = [a[:, k] for k in range(6)]
    l00 = np.sqrt(a[0])
    l10, l20 = a[1] / l00, a[2] / l00
    l11 = np.sqrt(a[3] - l10 * l10)
    l21 = (a[4] - l20 * l10) / l11
    l22 = np.sqrt(a[5] - l20 * l20 - l21 * l21)
    m00, m11, m22 = 1.0 / l00, 1.0 / l11, 1.0 / l22
    m10 = -l10 * m00 * m11
    m21 = -l21 * m11 * m22
    m20 = -(l20 * m00 + l21 * m10) * m22
    return np.stack([m00 * m00 + m10 * m10 + m20 * m20, m10 * m11 + m20 * m21, m20 * m22, m11 * m11 + m21 * m21, m21 * m22,
                     m22 * m22], axis=1)


def wave_ranges(ptr, N, P):
    """TableBuild::wave_ranges: cut at point boundaries, at least max(64, N / (waves of the device)) observations each."""
    T = max(64, -(-N // (N_CU * WAVES)))
    out, start = [], 0
    for p in range(P):
        endp = int(ptr[p + 1])
        if endp - start >= T or (p == P - 1 and endp > start):
            out.append((start, endp))
            start = endp
    return out


class Emulation:
    """Stands in for a Backend where there is no device: residual_jacobian, normal_blocks, form and step_products of one
    problem in plain float64 numpy from the fp64 oracle's blocks, with the fp32 roundings of the named operands of 32-bit
    storage (the stored Jc, Jp, r and t1; the pixels) and the device's summation structure (the window walk of k_backsub
    with both of its branches, seg_reduce_serial, wave_sum, the waves of a workgroup, the partial rows, the camera slice
    and its trips; k_jdot's grid-stride lanes).  `plant`: one of PLANTS, an error a check has to reject."""

    def __init__(self, orc, pb, bits=64, options=None, fixed=(), plant=None):
        assert plant is None or plant in PLANTS
        o = dict(options or {})
        self.pb, self.bits, self.plant, self.fixed = pb, bits, plant, tuple(fixed)
        C, P = pb.n_cameras, pb.n_points
        self.ci, self.pi = np.asarray(pb.camera_indices, dtype=np.int64), np.asarray(pb.point_indices, dtype=np.int64)
        assert np.all(np.diff(self.pi) >= 0), "the emulation takes the caller's order for the point-major order"
        self.N = len(self.ci)
        self.forms = {"lds_vec": int(C <= VEC and o.get("vec_lds", -1) != 0),
                      "jfree": int(o.get("jfree", -1) == 1 and C <= eb.lds_limit(eb.kernel_constant("kCamRow"))), "rc_cons": 0}
        uv = np.asarray(pb.points_2d, dtype=np.float64)
        if bits == 32:
            uv = uv.astype(F32).astype(np.float64)
        self.r, self.Jc, self.Jp = orc.jacobian_blocks(pb.x0, C, P, self.ci, self.pi, uv, pb.K)
        self.nb = orc.normal_blocks(self.r, self.Jc, self.Jp, C, P, self.ci, self.pi)
        for c in self.fixed:                                 # a camera held still: no U, no g_c (scale 1, gradient 0)
            self.nb.U[c], self.nb.gc[c] = 0.0, 0.0
        self.ptr = np.concatenate([[0], np.cumsum(np.bincount(self.pi, minlength=P))])
        self.ranges = wave_ranges(self.ptr, self.N, P)
        self.grid = -(-len(self.ranges) // WAVES)            # workgroups of k_backsub
        self.per = -(-6 * C // self.grid)                    # its camera slice per workgroup

    def form(self, name):
        return self.forms[name]

    def _stored(self, a):
        return a.astype(F32).astype(np.float64) if self.bits == 32 else a

    def residual_jacobian(self, x):
        assert np.array_equal(x, self.pb.x0)
        return self._stored(self.r).ravel(), self._stored(self.Jc), self._stored(self.Jp)

    def normal_blocks(self, x):
        assert np.array_equal(x, self.pb.x0)
        return eb.upper(self.nb.U), eb.upper(self.nb.V), self.nb.gc.copy(), self.nb.gp.copy()

    def step_products(self, x, sg, dc, dp_diag):
        assert np.array_equal(x, self.pb.x0)
        C, P, N, ci, pi, ptr, plant = self.pb.n_cameras, self.pb.n_points, self.N, self.ci, self.pi, self.ptr, self.plant
        jfree = self.forms["jfree"] == 1
        Jc, Jp = (self.Jc, self.Jp) if jfree else (self._stored(self.Jc), self._stored(self.Jp))   # recomputed in fp64 | load_blocks
        sg, dc, dp_diag = (np.asarray(a, dtype=np.float64).ravel() for a in (sg, dc, dp_diag))
        sgc, sgp = sg[:6 * C].reshape(C, 6), sg[6 * C:].reshape(P, 3)
        # ---- k_jdot ----
        t1 = np.zeros((N, 2))
        for k in range(6):
            t1 = t1 + Jc[:, :, k] * sgc[ci, k][:, None]
        for k in range(3):
            t1 = t1 + Jp[:, :, k] * sgp[pi, k][:, None]
        t1_stored = self._stored(t1)                         # store_pair
        sq = t1_stored if plant == "g11_from_stored_t1" else t1
        term = sq[:, 0] * sq[:, 0] + sq[:, 1] * sq[:, 1]
        threads = min(max(-(-N // 1024), 1), N_CU) * 1024
        trips = -(-N // threads)
        lanes = np.zeros(threads)
        padded = np.concatenate([term, np.zeros(trips * threads - N)]).reshape(trips, threads)
        for k in range(trips):
            lanes = lanes + padded[k]
        waves = _wave_sum(lanes.reshape(-1, WAVES, 64))      # (workgroups, waves)
        g11 = 0.0
        for b in range(waves.shape[0]):                      # the partial rows in the order the host sums them
            s = 0.0
            for w in range(WAVES):
                s += waves[b, w]
            g11 += s
        # ---- k_point_prep, k_update_scale: Vinv; gradient and inverse column scale of x ----
        a6 = eb.upper(self.nb.V).astype(np.float64)
        a6[:, 0], a6[:, 3], a6[:, 5] = a6[:, 0] + dp_diag[0::3], a6[:, 3] + dp_diag[1::3], a6[:, 5] + dp_diag[2::3]
        vinv = _chol3_inverse(a6)
        d = np.concatenate([np.einsum("cii->ci", self.nb.U).ravel(), np.einsum("pii->pi", self.nb.V).ravel()])
        si = np.where(d > 0, 1.0 / np.sqrt(np.where(d > 0, d, 1.0)), 1.0)
        gp = self.nb.gp
        g = np.concatenate([self.nb.gc.ravel(), gp.ravel()])
        # ---- k_transpose / the LDS staging: the camera-major copy of the step the sweep reads ----
        planes = dc.reshape(C, 6).T.copy().ravel()           # what the entry uploads: plane-major [6][C]
        in_lds = self.forms["lds_vec"] == 1 and not jfree
        vv = planes if (plant == "plane_major_dc" and not in_lds) else planes.reshape(6, C).T.copy().ravel()
        vvc = vv.reshape(C, 6)
        # ---- k_backsub ----
        t1_read = t1 if plant == "g12_from_unrounded_t1" else t1_stored      # load_pair
        acc = np.zeros((self.grid * WAVES, 64, 10))          # per lane: G12, G22, q5..q8 points, q5..q8 cameras
        dp = np.full((P, 3), np.nan)
        lane = np.arange(64)

        def jcv(j):
            if plant == "t_in_fp32":
                t = np.zeros((len(j), 2), dtype=F32)
                for k in range(6):
                    t = (t + (Jc[j, :, k] * vvc[ci[j], k][:, None]).astype(F32)).astype(F32)
                return t.astype(np.float64)
            t = np.zeros((len(j), 2))
            for k in range(6):
                t = t + Jc[j, :, k] * vvc[ci[j], k][:, None]
            return t

        def y_of(j, t):
            return Jp[j, 0, :] * t[:, 0][:, None] + Jp[j, 1, :] * t[:, 1][:, None]

        def solve_point(p, y):
            b = -gp[p] - y
            v = vinv[p]
            z = np.stack([v[:, 0] * b[:, 0] + v[:, 1] * b[:, 1] + v[:, 2] * b[:, 2],
                          v[:, 1] * b[:, 0] + v[:, 3] * b[:, 1] + v[:, 4] * b[:, 2],
                          v[:, 2] * b[:, 0] + v[:, 4] * b[:, 1] + v[:, 5] * b[:, 2]], axis=1)
            dp[p] = z
            return z

        def point_dots(w, ln, p, z):
            s3 = si[6 * C:].reshape(P, 3)[p]
            for k in range(3):
                ge, pe, s_ = gp[p, k], z[:, k], s3[:, k]
                acc[w, ln, 2] += ge * pe
                acc[w, ln, 3] += (pe * s_) * (pe * s_)
                acc[w, ln, 4] += (ge / (s_ * s_)) * pe
                acc[w, ln, 5] += pe * pe

        def gram(w, ln, j, t, z):
            a0 = ((t[:, 0] + Jp[j, 0, 0] * z[:, 0]) + Jp[j, 0, 1] * z[:, 1]) + Jp[j, 0, 2] * z[:, 2]
            a1 = ((t[:, 1] + Jp[j, 1, 0] * z[:, 0]) + Jp[j, 1, 1] * z[:, 1]) + Jp[j, 1, 2] * z[:, 2]
            acc[w, ln, 0] += t1_read[j, 0] * a0 + t1_read[j, 1] * a1
            acc[w, ln, 1] += a0 * a0 + a1 * a1

        self.long_runs = 0
        for w, (pos, end) in enumerate(self.ranges):
            while pos < end:
                i = pos + lane
                inn = i < end
                p = pi[np.where(inn, i, pos)]
                sb, se = ptr[p], ptr[p + 1]
                n_take = int(np.sum(inn & (se <= pos + 64)))
                if n_take == 0:                              # a run longer than the window: a step of its own
                    run_end, pp = int(se[0]), int(p[0])
                    starts = list(range(pos, run_end, 64))
                    if plant == "long_run_tail_dropped" and run_end - starts[-1] < 64:
                        starts = starts[:-1]
                    self.long_runs += 1
                    y = np.zeros((64, 3))
                    for j0 in starts:
                        j = j0 + lane
                        m = j < run_end
                        y[m] = y[m] + y_of(j[m], jcv(j[m]))
                    ys = np.stack([_wave_sum(y[:, k]) for k in range(3)])[None, :]
                    z = solve_point(np.array([pp]), ys)
                    point_dots(w, np.array([0]), np.array([pp]), z)
                    for j0 in starts:
                        j = j0 + lane
                        m = j < run_end
                        gram(w, lane[m], j[m], jcv(j[m]), np.repeat(z, int(m.sum()), axis=0))
                    pos = run_end
                    continue
                act = lane < n_take
                j = i[act]
                t = jcv(j)
                y = np.zeros((64, 3))
                y[act] = y_of(j, t)
                ys = _seg_reduce(y, np.where(act, sb, -1 - lane))
                head = act & (i == sb)
                zl = np.zeros((64, 3))
                zl[head] = solve_point(p[head], ys[head])
                point_dots(w, lane[head], p[head], zl[head])
                gram(w, lane[act], j, t, zl[(lane - (i - sb))[act]])
                pos += n_take
        # the camera slice: `per` elements per workgroup, thread t takes t, t + 1024, ...
        n_trips = -(-self.per // (64 * WAVES))
        self.slice_trips = n_trips
        for b in range(self.grid):
            for trip in range(1 if plant == "camera_slice_one_trip" else n_trips):
                tt = np.arange(trip * 64 * WAVES, min((trip + 1) * 64 * WAVES, self.per))
                e = b * self.per + tt
                tt, e = tt[e < 6 * C], e[e < 6 * C]
                th = tt - trip * 64 * WAVES
                w_, ln, pe, s_ = b * WAVES + th // 64, th % 64, vv[e], si[e]
                acc[w_, ln, 6] += g[e] * pe
                acc[w_, ln, 7] += (pe * s_) * (pe * s_)
                acc[w_, ln, 8] += sg[e] * pe
                acc[w_, ln, 9] += pe * pe
        rows = _wave_sum(np.moveaxis(acc, 1, 2)).reshape(self.grid, WAVES, 10)
        sums = np.zeros(10)
        for b in range(self.grid):
            a = np.zeros(10)
            for w in range(WAVES):
                a = a + rows[b, w]
            sums = sums + a
        return {"t1": t1_stored, "g11": g11, "dp": dp, "sums": sums, "g": g, "si": si}
