"""fp32 storage and the mixed-precision Schur product entry by entry: the references and bounds of
test_gpu_entries32.py and of the fp32 half of test_host_entry_bounds.py, on the conventions of entry_bounds.py
(longdouble references, k counted from the kernel source, A the abs-value evaluation, nothing taken from a device
except where a layer's reference takes the previous layer's FETCHED values as exact operands, the precedent of
test_gpu_rc_consumers.py).

The contract of the mixed-precision product (ba_kernels.hpp, MixedPrep): its OPERANDS are fp32 and everything computed
from them is fp64.  The only fp32 roundings are of named operands --
    rt32   = fl32(R) | fl32(T - o)              k_mixed_prep / k_prep (mixed_prep_camera)
    rec32  = fl32(X - o) | fl32(z)              mixed_prep_point; store_z of k_point_sweep_rc32
    a'     = fl32(u_w - b (w x u_w) + c (w x (w x u_w))),  u_T = fl32(v_T)      put_au / k_rc_table32; pass B rounds its own
-- so a reference that rounds the same operands and does the rest in longdouble agrees with the device to fp64
rounding error, and an fp32 STORE agrees with float32(reference) bit for bit except where the reference lies within its
fp64 bound of a rounding boundary of fp32 (a "tie entry": fl32_interval then holds two floats and either is accepted).

Roundings of the rows j_k from the operands (contrib of k_point_sweep_rc32, the MIXED branch of k_cam_schur and
k_cam_schur_w: the same expressions in R | T - o, X - o and K; a rounded R is not a rotation, so nothing is re-derived
from w), both factors of a product counted as entry_bounds._mul does for the deeper quantities:
    v = X - T: 1;  q = R v: (0 + 1 + 1) and two additions: 4;  p = K q: 5 and two additions: 7;  iz = 1 / p_z: 8;
    pk = p_k iz: 7 + 8 + 1 = 16;  b = (K_k - pk K_3) iz: 17, 18, then 18 + 8 + 1 = 27;  j = b R, three terms: 28 and two
    additions: 30 (OperandRows.k_j).
Pass A:  g = v x a' + u_T: product 2, subtraction 3, addition 4;  t_k = -(j_k . g): 30 + 4 + 1 and two additions: 37;
    y += j_k t_k: 30 + 37 + 1 and two additions: 70, then the run (run_roundings_sweep);  z = Vinv y_p, Vinv from the
    FETCHED V_p (its own test holds it to its bound): the diagonal added, 1, and chol3_inverse, CHOL_ROUNDINGS, passed
    on by |Vinv| . |Vinv|; three products and two additions.
Pass B on fp32 records (z an operand):  h = z + (v x a' + u_T): 5;  u_k = -(j_k . h): 38;  q = sum_k u_k j_k: 71;  the
    camera's sums of q x v (74) and q by the structure of the pass (entry_bounds.Structure.pass_b); the rotation Jacobian
    applied to the summed M with the fp64 w, b, c of the camera table as schur_product counts it; dc v: 2.
Pass B with pcg_mixed_b = 0 (fp64 records): pass A from the rounded operands chained in longdouble into pass B from x,
    k_z as counted above.
The stored fp32 Jacobian (round_blocks): the J that residual_jacobian fetches is the operand of BOTH passes;
    t = Jc v: six products added to 0: 7;  y_p: 0 + 7 + 1 and two additions, then the run;  z as above;
    u = -(Jp z) + Jc v: 0 + k_z + 1, two additions, six more;  a += Jc^T u: 0 + k_u + 1 and two additions, the camera's
    sum; dc v: 2."""
import numpy as np

import entry_bounds as eb
from entry_bounds import LD, _add, _cross, _group_max, _mul, _xabs, run_roundings_sweep

F32 = np.float32


def fl32(a):
    """float32 of a longdouble (or double) array by ONE rounding to nearest."""
    return np.asarray(a).astype(F32)


def fl32_interval(ref, bnd):
    """The floats an fp32 store of a value within `bnd` of `ref` may hold -> (lo, hi, tie): float32(ref - bnd),
    float32(ref + bnd) and where they differ (the tie entries)."""
    ref, bnd = np.asarray(ref, dtype=LD), np.asarray(bnd, dtype=LD)
    lo, hi = (ref - bnd).astype(F32), (ref + bnd).astype(F32)
    return lo, hi, lo != hi


def accepted32(got, ref, bnd):
    """`got` entry by entry: a float32 value inside fl32_interval(ref, bnd) -> (accepted, tie)."""
    g = np.asarray(got, dtype=np.float64).reshape(np.shape(ref))
    lo, hi, tie = fl32_interval(ref, bnd)
    ok = (g.astype(F32).astype(np.float64) == g) & (lo.astype(np.float64) <= g) & (g <= hi.astype(np.float64))
    return ok, tie


def ratio32(got, ref, bnd):
    """Largest |got - ref| / (bound + half an ulp of fp32 at ref): what an fp32 store of a value inside its bound stays below 1 of."""
    ref = np.asarray(ref, dtype=LD)
    a = np.abs(ref).astype(F32)
    half_ulp = (np.nextafter(a, F32(np.inf)) - a).astype(LD) / 2
    err = np.abs(np.asarray(got, dtype=np.float64).reshape(ref.shape).astype(LD) - ref)
    return float((err / (np.asarray(bnd, dtype=LD) + half_ulp)).max()) if err.size else 0.0


def origin_of(x, C, P):
    """upload_x's origin of the fp32 operands: the mean of every max(1, P // 1024)-th point of x, a serial double sum in
    index order (a plain loop: numpy's pairwise sum gives other bits); a non-finite result gives 0."""
    pts = np.asarray(x, dtype=np.float64)[6 * C:]
    stride = max(1, P // 1024)
    sx = sy = sz = 0.0
    cnt = 0
    for q in range(0, P, stride):
        sx += float(pts[3 * q])
        sy += float(pts[3 * q + 1])
        sz += float(pts[3 * q + 2])
        cnt += 1
    if cnt == 0:
        return np.zeros(3)
    o = np.array([sx / cnt, sy / cnt, sz / cnt])
    return o if np.isfinite(o[0] + o[1] + o[2]) else np.zeros(3)


def operands_from_x(lin, x, v):
    """The fp32 operands of (x, v) -> dict: origin (3); rt (C, 12) longdouble reference of rt32 with its bound rt_bnd
    (R: the camera table's k_R eps A(R); T - o: float64(T) - o as mixed_prep_camera subtracts, exact, bound 0); X32 (P, 3) float32 = float32(float64(X) - o),
    exact; a32 (C, 3) = fl32 of _a_prime with a_tie, where its interval holds two floats; uT32 (C, 3) = float32(v_T)."""
    C, P = lin.C, lin.P
    x = np.asarray(x, dtype=np.float64)
    T, X = x[:6 * C].reshape(C, 6)[:, 3:], x[6 * C:].reshape(P, 3)
    o = origin_of(x, C, P)
    rt = np.concatenate([lin.R.reshape(C, 9), (T - o).astype(LD)], axis=1)      # (T - o: the kernel's own double subtraction)
    rt_bnd = np.concatenate([eb.bound(lin.k_R, lin.Ra).reshape(C, 9), np.zeros((C, 3), dtype=LD)], axis=1)
    vc = np.asarray(v, dtype=np.float64).reshape(C, 6)
    ap, apa, k_ap = lin._a_prime(vc.astype(LD))
    _, _, a_tie = fl32_interval(ap, eb.bound(k_ap, apa))
    return {"origin": o, "rt": rt, "rt_bnd": rt_bnd, "X32": (X - o).astype(F32), "T32": (T - o).astype(F32),
            "a32": fl32(ap), "a_tie": a_tie, "uT32": vc[:, 3:].astype(F32)}


def point_inverses_from(V, dp, dt=LD):
    """Vinv = (V + diag dp)^-1 with the fetched V (P, 3, 3) an exact operand: the diagonal's addition and chol3_inverse,
    passed on by |Vinv| . |Vinv| (entry_bounds.Linearisation.point_inverses without the error of V)."""
    V = np.asarray(V, dtype=np.float64).astype(dt)
    P = V.shape[0]
    A = V + np.einsum("pi,ij->pij", np.asarray(dp, dtype=np.float64).reshape(P, 3).astype(dt), np.eye(3, dtype=dt))
    Vinv = eb._inv3(A)
    aV = np.abs(Vinv)
    return {"Vinv": Vinv, "Vinva": np.einsum("pij,pjk,pkl->pil", aV, np.abs(A), aV), "k_Vinv": np.full(P, 1.0 + eb.CHOL_ROUNDINGS)}


def full3(V6):
    """(P, 6) packed upper triangles -> (P, 3, 3)."""
    V6 = np.asarray(V6).reshape(-1, 6)
    out = np.empty((V6.shape[0], 3, 3), dtype=V6.dtype)
    iu = np.triu_indices(3)
    out[:, iu[0], iu[1]] = V6
    out[:, iu[1], iu[0]] = V6
    return out


class OperandRows:
    """The rows j (N, 2, 3) of d r/d X, v = (X - o) - (T - o) and their abs-value companions from the fp32 operands taken
    as exact: R (C, 3, 3), T (C, 3), X (P, 3) -- the module's header has the expressions and the count k_j = 30."""

    def __init__(self, lin, K, R, T, X, dt=LD):
        ci, pi = lin.ci, lin.pi
        K = np.asarray(K, dtype=np.float64).astype(dt)
        Ka = np.abs(K)
        R, T, X = (np.asarray(a).astype(dt) for a in (R, T, X))
        Rn, Ran = R[ci], np.abs(R[ci])
        self.v, self.va, self.k_v = X[pi] - T[ci], np.abs(X[pi]) + np.abs(T[ci]), 1
        q, qa = np.einsum("nij,nj->ni", Rn, self.v), np.einsum("nij,nj->ni", Ran, self.va)
        p, pa = q @ K.T, qa @ Ka.T
        iz, iza = 1 / p[:, 2], pa[:, 2] / p[:, 2] ** 2
        u, ua = p[:, :2] * iz[:, None], pa[:, :2] * iza[:, None]
        A = (K[None, :2, :] - u[:, :, None] * K[None, 2:3, :]) * iz[:, None, None]
        self.j = np.einsum("nkm,nmi->nki", A, Rn)
        self.js = np.abs(self.j)
        k_q = _mul(0, self.k_v) + 2
        k_p = _mul(0, k_q) + 2
        k_iz = k_p + 1
        k_u = _mul(k_p, k_iz)
        self.k_j = _mul(_mul(_mul(k_u, 0) + 1, k_iz), 0) + 2
        assert self.k_j == 30


def pass_a(lin, rows, pv, a32, uT32, dt=LD):
    """z = Vinv sum_i j_i^T t_i, t_k = -(j_k . (v x a' + u_T)) of k_point_sweep_rc32 -> z, za (P, 3), k_z (P)."""
    ci, pi = lin.ci, lin.pi
    a, uT = np.asarray(a32).astype(dt), np.asarray(uT32).astype(dt)
    g, ga = _cross(rows.v, a[ci]) + uT[ci], _xabs(rows.va, np.abs(a[ci])) + np.abs(uT[ci])
    k_g = _mul(rows.k_v, 0) + 2
    t, ta = -np.einsum("nki,ni->nk", rows.j, g), np.einsum("nki,ni->nk", rows.js, ga)
    k_t = _mul(rows.k_j, k_g) + 2
    yp, ypa = np.zeros((lin.P, 3), dtype=dt), np.zeros((lin.P, 3), dtype=dt)
    np.add.at(yp, pi, np.einsum("nki,nk->ni", rows.j, t))
    np.add.at(ypa, pi, np.einsum("nki,nk->ni", rows.js, ta))
    k_yp = _mul(rows.k_j, k_t) + 2 + run_roundings_sweep(lin.Lp)
    return {"z": np.einsum("pij,pj->pi", pv["Vinv"], yp), "za": np.einsum("pij,pj->pi", pv["Vinva"], ypa),
            "k_z": _mul(pv["k_Vinv"], k_yp) + 2, "t": t}


def pass_b(lin, st, j, js, k_j, v, va, k_v, ap, apa, k_ap, uT, z, za, k_z, dc, vc, dt=LD, drop=None):
    """y = sum Jc^T (Jc v - Jp z) + dc v in pass B's own form (k_cam_schur / k_cam_schur_w, exact blocks) from the rows j,
    v = X - T, a', u_T and z, each with its count (0 for an operand) -> y, ya (C, 6), k_y (C, 6), and the per-observation
    u (N, 2).  drop: an observation left out of the camera sums (a planted error)."""
    C, ci, pi = lin.C, lin.ci, lin.pi
    k_ap = np.broadcast_to(np.asarray(k_ap, dtype=np.float64), (C,))
    k_z = np.broadcast_to(np.asarray(k_z, dtype=np.float64), (lin.P,))
    g, ga = _cross(v, ap[ci]) + uT[ci], _xabs(va, apa[ci]) + np.abs(uT[ci])
    k_g = _mul(k_v, k_ap[ci]) + 2
    h, ha, k_h = z[pi] + g, za[pi] + ga, np.maximum(k_z[pi], k_g) + 1
    u, ua, k_u = -np.einsum("nki,ni->nk", j, h), np.einsum("nki,ni->nk", js, ha), _mul(k_j, k_h) + 2
    q, qa, k_q = np.einsum("nk,nki->ni", u, j), np.einsum("nk,nki->ni", ua, js), _mul(k_u, k_j) + 2
    keep = np.ones(len(ci), dtype=bool)
    if drop is not None:
        keep[drop] = False
    M, Ma, S, Sa = (np.zeros((C, 3), dtype=dt) for _ in range(4))
    np.add.at(M, ci[keep], _cross(q, v)[keep])
    np.add.at(Ma, ci[keep], _xabs(qa, va)[keep])
    np.add.at(S, ci[keep], q[keep])
    np.add.at(Sa, ci[keep], qa[keep])
    k_S = _group_max(k_q, ci, C) + st.pass_b
    k_M = _group_max(_mul(k_q, k_v) + 1, ci, C) + st.pass_b
    w, wa, b, c, ca = lin.w.astype(dt), lin.wa.astype(dt), lin.b.astype(dt), lin.c.astype(dt), lin.ca.astype(dt)
    c0, c0a = _cross(M, w), _xabs(Ma, wa)
    rot = -(M - b[:, None] * c0 + c[:, None] * _cross(c0, w))
    rota = Ma + b[:, None] * c0a + ca[:, None] * _xabs(c0a, wa)
    k_w = _add(_add(k_M, _mul(lin.k_b, k_M + 2)), _mul(lin.k_c, k_M + 4))
    dcc, vcc = np.asarray(dc, dtype=np.float64).reshape(C, 6).astype(dt), np.asarray(vc, dtype=np.float64).reshape(C, 6).astype(dt)
    return {"y": np.concatenate([rot, -S], axis=1) + dcc * vcc, "ya": np.concatenate([rota, Sa], axis=1) + np.abs(dcc * vcc),
            "k_y": np.concatenate([np.repeat(k_w[:, None], 3, axis=1), np.repeat(k_S[:, None], 3, axis=1)], axis=1) + 2,
            "u": u}


def mixed_product(lin, st, K, dc, dp, v, rt32, X32, V, mixed_b=True, z32=None, a32=None, uT32=None, dt=LD, rows64=None,
                  drop=None):
    """The references of one mixed-precision product: pass A from the operands rt32 (C, 12), X32 (P, 3) (fetched, or
    emulated by operands_from_x), the emulated a', u_T and the fetched V (P, 3, 3) -> "a" (pass_a's dict); pass B
    -> "b" (pass_b's dict): on fp32 records from z32 (fetched; None: fl32 of pass A's z, for the tests without a device),
    or, mixed_b false, on the fp64 records: pass A's unrounded z chained into pass B from x.  dt = float64 with rows64
    (Jp (N, 2, 3) of the fp64 oracle): the same in plain double arithmetic, the "fp64 oracle" of the host tests."""
    C = lin.C
    vc = np.asarray(v, dtype=np.float64).reshape(C, 6)
    if a32 is None:
        a32 = fl32(lin._a_prime(vc.astype(LD))[0])
    if uT32 is None:
        uT32 = vc[:, 3:].astype(F32)
    rt32 = np.asarray(rt32, dtype=F32).reshape(C, 12)
    pv = point_inverses_from(V, dp, dt)
    rows = OperandRows(lin, K, rt32[:, :9].reshape(C, 3, 3), rt32[:, 9:], np.asarray(X32, dtype=F32), dt)
    A = pass_a(lin, rows, pv, a32, uT32, dt)
    if mixed_b:
        zz = (fl32(A["z"]) if z32 is None else np.asarray(z32, dtype=F32)).astype(dt)
        ap, uT = np.asarray(a32).astype(dt), np.asarray(uT32).astype(dt)
        B = pass_b(lin, st, rows.j, rows.js, rows.k_j, rows.v, rows.va, rows.k_v, ap, np.abs(ap), 0.0, uT, zz, np.abs(zz), 0.0,
                   dc, vc, dt, drop)
    else:
        ap, apa, k_ap = lin._a_prime(vc.astype(LD))
        j = lin.Jp if rows64 is None else np.asarray(rows64, dtype=np.float64)
        B = pass_b(lin, st, j.astype(dt), lin.Jps.astype(dt), lin.ka_jp, lin.v.astype(dt), lin.va.astype(dt), 1, ap.astype(dt),
                   apa.astype(dt), k_ap, vc[:, 3:].astype(dt), A["z"], A["za"], A["k_z"], dc, vc, dt, drop)
    return {"a": A, "b": B, "rows": rows}


def stored_product(lin, st, Jc, Jp, V, dc, dp, v, dt=LD):
    """y = S v with the stored fp32 Jacobian (round_blocks): the fetched Jc (N, 2, 6), Jp (N, 2, 3) are the operands of
    pass A (k_point_sweep) and of pass B (k_cam_schur<0, ROUND>, which claims to round its recomputed blocks alike)."""
    C, P, ci, pi = lin.C, lin.P, lin.ci, lin.pi
    Jc, Jp = np.asarray(Jc, dtype=np.float64).astype(dt), np.asarray(Jp, dtype=np.float64).astype(dt)
    vc, dcc = np.asarray(v, dtype=np.float64).reshape(C, 6).astype(dt), np.asarray(dc, dtype=np.float64).reshape(C, 6).astype(dt)
    pv = point_inverses_from(V, dp, dt)
    t, ta, k_t = np.einsum("nki,ni->nk", Jc, vc[ci]), np.einsum("nki,ni->nk", np.abs(Jc), np.abs(vc[ci])), 0 + 1 + 6
    yp, ypa = np.zeros((P, 3), dtype=dt), np.zeros((P, 3), dtype=dt)
    np.add.at(yp, pi, np.einsum("nki,nk->ni", Jp, t))
    np.add.at(ypa, pi, np.einsum("nki,nk->ni", np.abs(Jp), ta))
    k_yp = _mul(0, k_t) + 2 + run_roundings_sweep(lin.Lp)
    z, za = np.einsum("pij,pj->pi", pv["Vinv"], yp), np.einsum("pij,pj->pi", pv["Vinva"], ypa)
    k_z = _mul(pv["k_Vinv"], k_yp) + 2
    u = t - np.einsum("nki,ni->nk", Jp, z[pi])
    ua = ta + np.einsum("nki,ni->nk", np.abs(Jp), za[pi])
    k_u = _mul(0, k_z[pi]) + 2 + 6
    y, ya = np.zeros((C, 6), dtype=dt), np.zeros((C, 6), dtype=dt)
    np.add.at(y, ci, np.einsum("nki,nk->ni", Jc, u))
    np.add.at(ya, ci, np.einsum("nki,nk->ni", np.abs(Jc), ua))
    k_y = _group_max(_mul(0, k_u) + 2, ci, C) + st.pass_b + 2
    return {"y": y + dcc * vc, "ya": ya + np.abs(dcc * vc), "k_y": np.repeat(k_y[:, None], 6, axis=1)}


# ---- the problems and cases ------------------------------------------------------------------------------------------------
SHIFT = 4.0e6                                                # the scene of test_mixed_precision_schur_product, 4000 km out


def problem32(name, orc):
    """entry_bounds.problem, and `<name>_shifted`: cameras and points moved by SHIFT along every axis."""
    if name.endswith("_shifted"):
        args, x = eb.problem(name[:-len("_shifted")], orc)
        C = args[0]
        x = np.array(x, dtype=np.float64)
        x[:6 * C].reshape(C, 6)[:, 3:] += SHIFT
        x[6 * C:] += SHIFT
        return args, x
    if name.startswith("origin_"):                           # P >= 2048: the origin's sample takes every second point or fewer
        if name not in eb._CACHE:
            import sfmba
            pb = sfmba.make_problem(20, int(name[7:]), 8000, seed=1)
            eb._CACHE[name] = (pb.args, pb.x0)
        return eb._CACHE[name]
    return eb.problem(name, orc)


def linearisation32(name, orc, bits):
    """The Linearisation of a problem as the storage mode sees its pixels: float32(uv) with 32-bit storage."""
    key = ("lin32", name, bits)
    if key not in eb._CACHE:
        args, x = problem32(name, orc)
        uv = np.asarray(args[4], dtype=np.float64)
        if bits == 32:
            uv = uv.astype(F32).astype(np.float64)
        eb._CACHE[key] = eb.Linearisation(args[0], args[1], args[2], args[3], uv, args[5], x)
    return eb._CACHE[key]


def operands32(lin, st):
    """dc, dp, v of a case (entry_bounds.operands) with the first seed whose emulated a' has no tie entry: a' is not
    fetched, so its emulation must not depend on the device's last bits -> (dc, dp, v, seed)."""
    for seed in range(16):
        dc, dp, v = eb.operands(lin, st, seed)
        ap, apa, k_ap = lin._a_prime(v.reshape(lin.C, 6).astype(LD))
        if not fl32_interval(ap, eb.bound(k_ap, apa))[2].any():
            return dc, dp, v, seed
    raise RuntimeError("no seed without a tie entry in a'")


_M = dict(mixed=1, mixed_b=1, sweep_rc=1, sweep_rc_g=0, xcd_b=0, cam_multi=0, pcg_fused=1, round_blocks=0)
_RC = eb.kernel_constant("kRcMaxCams")
# name -> (problem, storage bits, debug options, forms that form() must report)
MIXED_CASES = {
    "default": ("hand_built", 32, {}, _M),
    "sweep_rc_g": ("hand_built", 32, {"sweep_rc": 2}, dict(_M, sweep_rc=0, sweep_rc_g=1)),
    "cam_chunk64": ("hand_built", 32, {"cam_chunk": 64}, dict(_M, cam_multi=1)),
    "xcd": ("hand_built", 32, {"xcd_chunks": 1}, dict(_M, xcd_b=1)),
    "mixed_b0": ("hand_built", 32, {"pcg_mixed_b": 0}, dict(_M, mixed_b=0)),
    "mixed_b0_xcd": ("hand_built", 32, {"pcg_mixed_b": 0, "xcd_chunks": 1}, dict(_M, mixed_b=0, xcd_b=1)),
    "mixed_b0_sweep_rc_g": ("hand_built", 32, {"pcg_mixed_b": 0, "sweep_rc": 2}, dict(_M, mixed_b=0, sweep_rc=0, sweep_rc_g=1)),
    "fp64_storage": ("hand_built", 64, {"pcg_mixed": 1}, _M),
    "fused_1024": ("schur_1024", 32, {}, _M),
    "unfused_1025": ("schur_1025", 32, {}, dict(_M, pcg_fused=0)),
    "lds_table": ("schur_%d" % _RC, 32, {}, dict(_M, pcg_fused=0)),
    "l2_table": ("schur_%d" % (_RC + 1), 32, {}, dict(_M, sweep_rc=0, sweep_rc_g=1, pcg_fused=0)),
    "shifted": ("hand_built_shifted", 32, {}, _M),
}
_S = dict(mixed=0, mixed_b=0, sweep_rc=0, sweep_rc_g=0, xcd_b=0, cam_multi=0, pcg_fused=1, round_blocks=1)
STORED_CASES = {
    "lds_vec": ("hand_built", 32, {"sweep_rc": 0}, dict(_S, lds_vec=1)),
    "l2_vec": ("hand_built", 32, {"sweep_rc": 0, "vec_lds": 0}, dict(_S, lds_vec=0, pcg_fused=0)),
}
ORIGIN_POINTS = 2600                                          # stride 2

# The tie entries (fl32_interval holds two floats) of any array of any case: a cap, not a measurement -- k eps64 A / ulp32
# is near 1e-6 of the entries.
TIE_CAP = 1e-3


def case(name, orc, cases=None):
    """-> (args, x, lin, st, (dc, dp, v), options, forms, bits) of a case."""
    problem, bits, options, forms = (cases or MIXED_CASES)[name]
    args, x = problem32(problem, orc)
    lin = linearisation32(problem, orc, bits)
    key = ("st32", problem, tuple(sorted(options.items())))
    if key not in eb._CACHE:
        eb._CACHE[key] = eb.Structure(args[0], args[1], np.asarray(args[2]), np.asarray(args[3]), options)
    st = eb._CACHE[key]
    return args, x, lin, st, operands32(lin, st)[:3], options, forms, bits
