"""One outer iteration layer by layer: references and bounds for what `Backend.iteration_state()` fetches, shared by
test_gpu_iteration.py, test_host_iteration.py and tools/gen_iteration_golden.py.  Host only.

Every layer takes the FETCHED output of the layer before it as exact, so a reference is a few operations in
numpy.longdouble and a bound k eps A a few roundings (the conventions of entry_bounds.py: one rounding per operation,
eps = 2^-52, A the expression with every operand replaced by its absolute value):

  scale   U, V, g_c, g_p (sfmba_normal_blocks)  ->  si, g, sg, q0..q4            k_update_scale
  prep    the scalars, si, V, g_p, U             ->  radius, reg, eta, Dc, Vinv, e, Minv (precond = 0)   k_prep
  pcg     x, Dc, reg si_p^2, Minv, ctrl.iters    ->  dc, r, rz0, rz, the stop rule   every PCG form
  step    the scalars, x, sg, p                  ->  c1, c2, predicted, |step_h|, |step|, x_new   k_tr_step, k_step_table

The PCG amplifies rounding through its iterations, so its bound is not counted but MEASURED between the reference's own
two precisions (tools/gen_iteration_golden.py -> tests/golden/iteration_bounds.json), never against a device.

`replay` is the same iteration in plain float64 from x alone (the oracle's blocks, numpy's sums): what the host tests put
through the checks, what the generator measures, and -- with a `plant` -- a subtly wrong iteration."""
import json
import math
import os

import numpy as np

import entry_bounds as eb
from conftest import GOLDEN

LD, EPS = eb.LD, eb.EPS
POINT_SLOT = (12, 8, 9, 10, 11, 4, 5, 6, 7)      # slot of q0..q8 of the point slice (sfmba.hip: kPointSlot)
CAM_SLOT = 16                                    # q0..q8 of the camera slice
G11, G12, G22, REG, GH_PREV, ETA, STEP, SKIP, RADIUS = 1, 2, 3, 13, 14, 15, 25, 30, 31
DIAG_U, DIAG_V = (0, 6, 11, 15, 18, 20), (0, 3, 5)
DENSE_TOL_FACTOR = 0.1                           # sfmba.hip: kDenseTolFactor
BOUNDS_FILE = os.path.join(GOLDEN, "iteration_bounds.json")
PLANTS = ("beta_wrong_gamma", "dc_missing_from_w", "scale_forgets_max", "eta_never_clamped", "dp_missing_from_vinv",
          "held_scale_not_one")


def qsum(sc, q):
    """q of the whole parameter vector as host and device add it: point slice + camera slice."""
    return sc[POINT_SLOT[q]] + sc[CAM_SLOT + q]


def full_sym(packed, n):
    """(B, n (n + 1) / 2) packed upper triangles -> (B, n, n) symmetric."""
    iu = np.triu_indices(n)
    M = np.zeros((packed.shape[0], n, n), dtype=packed.dtype)
    M[:, iu[0], iu[1]] = packed
    M[:, iu[1], iu[0]] = packed
    return M


def _ratio(got, ref, bnd):
    return eb.ratio(got, np.asarray(ref, dtype=LD), np.asarray(bnd, dtype=LD))


def _exact(got, ref):
    return 0.0 if np.array_equal(np.asarray(got), np.asarray(ref)) else math.inf


# ---- scale ---------------------------------------------------------------------------------------------------------------
def check_scale(st, U, V, gc, gp, x, C, si_old=None, held=(), prefix=("si", "g", "sg")):
    """k_update_scale from the fetched blocks.  si = sqrt(diag) (one rounding; zero -> 1 on the first call, max(., si_old)
    afterwards: a maximum is exact), g the blocks' own bits, sg = g / (si si) from the fetched si (two roundings).
    -> {check: error / bound}; exact checks give 0 or inf."""
    si, g, sg = (np.asarray(st[k]) for k in prefix)
    d = np.concatenate([np.asarray(U)[:, DIAG_U].ravel(), np.asarray(V)[:, DIAG_V].ravel()]).astype(LD)
    ref = np.sqrt(d)
    if si_old is None:
        ref = np.where(d == 0, LD(1), ref)
    else:
        ref = np.maximum(ref, np.asarray(si_old).astype(LD))
    out = {"g": _exact(g, np.concatenate([np.asarray(gc).ravel(), np.asarray(gp).ravel()])),
           "si": _ratio(si, ref, EPS * ref)}
    if si_old is not None:                               # where the maximum holds an entry, it holds its bits
        kept = np.asarray(si_old) > np.sqrt(d).astype(np.float64) * (1 + 4 * EPS)
        out["si_running_max"] = _exact(si[kept], np.asarray(si_old)[kept])
    sl = si.astype(LD)
    out["sg"] = _ratio(sg, g.astype(LD) / (sl * sl), 2 * EPS * np.abs(g) / (sl * sl))
    for c in held:                                       # a held camera: no blocks, scale 1, no gradient
        e = slice(6 * c, 6 * c + 6)
        out["held"] = max(out.get("held", 0.0), _exact(si[e], np.ones(6)), _exact(g[e], np.zeros(6)), _exact(sg[e], np.zeros(6)))
    return out


def check_scale_sums(sc, st, x, C, prefix=("si", "g", "sg")):
    """q0..q4 of both slices from the fetched si, g, sg and x: q0 a maximum (exact); q1 = sum (g / si)^2 and
    q2 = sum (x si)^2 two roundings a term, q3 = sum x^2 and q4 = sum sg^2 one; a sum of n terms in any order is within
    n eps of the sum of its terms' magnitudes."""
    si, g, sg = (np.asarray(st[k]).astype(LD) for k in prefix)
    xl = np.asarray(x).astype(LD)
    out = {}
    for name, sl, slot in (("cam", slice(0, 6 * C), lambda q: CAM_SLOT + q), ("pt", slice(6 * C, None), lambda q: POINT_SLOT[q])):
        n = len(xl[sl])
        out[f"q0_{name}"] = _exact(sc[slot(0)], np.abs(np.asarray(st[prefix[1]])[sl]).max() if n else 0.0)
        terms = {1: ((g[sl] / si[sl]) ** 2, 2), 2: ((xl[sl] * si[sl]) ** 2, 2), 3: (xl[sl] ** 2, 1), 4: (sg[sl] ** 2, 1)}
        for q, (t, k) in terms.items():
            out[f"q{q}_{name}"] = _ratio(sc[slot(q)], t.sum(), (n + k) * EPS * t.sum())
    return out


# ---- prep ----------------------------------------------------------------------------------------------------------------
REG_ROUNDINGS = 7


def reg_from_scalars(a11, g11, Delta, reg_min, T=LD):
    """The Cauchy step of ba_oracle.trf_schur (lines 509-521), floor reg_min -> (reg, its abs-value evaluation).
    to_tr = Delta / sqrt(a11) (2 roundings); y = t (a t + b): 3 more, a cancelling sum; / Delta^2: 2: k = 7."""
    a11, g11, Delta = T(a11), T(g11), T(Delta)
    a, b = T(0.5) * g11, -a11
    if not a11 > 0:
        return T(reg_min), T(reg_min)
    to_tr = Delta / np.sqrt(a11)
    ys, ab = [T(0), to_tr * (a * to_tr + b)], [T(0), to_tr * (abs(a) * to_tr + abs(b))]
    if a != 0:
        ext = T(-0.5) * b / a
        if 0 < ext < to_tr:
            ys.append(ext * (a * ext + b))
            ab.append(ext * (abs(a) * ext + abs(b)))
    return max(-min(ys) / Delta ** 2, T(reg_min)), max(ab) / Delta ** 2


def eta_from(a11, prev, eta_min, eta_max, T=LD):
    """The forcing term of k_prep: eta_max at the start of a solve (prev = 0), else sqrt(a11 / prev) clamped to its limits."""
    if prev > 0 and a11 >= 0:
        return min(T(eta_max), max(T(eta_min), np.sqrt(T(a11) / T(prev))))
    return T(eta_max)


def check_prep(sc, st, V, gp, C, reg_min, eta_min, eta_max, prev=0.0, first=True, U=None, skip=()):
    """k_prep from the fetched scalars, si, V, g_p (and U where it inverts the camera blocks itself, precond = 0).
    radius: sqrt(q2) at a quick start (an addition and a root: 2), 1 when that is 0; later the host's own, read from slot 31.
    reg: REG_ROUNDINGS; eta: a division and a root (2), clamped; slot 14 afterwards holds a11, its own bits.
    Dc = (reg si) si: 2.  Vinv = (V + (reg s) s)^-1 by chol3_inverse: 3 roundings of the diagonal and CHOL_ROUNDINGS, passed
    on by |inv| A |inv|.  e = Vinv g_p from the fetched Vinv: a product and two additions (3).  Minv = (U + Dc)^-1 by
    spd6_inverse from the fetched Dc: 1 + SPD6_ROUNDINGS."""
    sc = np.asarray(sc)
    si = np.asarray(st["si"]).astype(LD)
    out = {}
    a11 = sc[8] + sc[CAM_SLOT + 1]                       # (one addition, the device's own: the same bits here)
    if first:
        d2 = sc[9] + sc[CAM_SLOT + 2]
        ref = np.sqrt(LD(d2)) if d2 != 0 else LD(1)
        out["radius"] = _ratio(sc[RADIUS], ref, 2 * EPS * ref)
    reg, rega = reg_from_scalars(a11, sc[G11], sc[RADIUS], reg_min)
    out["reg"] = _ratio(sc[REG], reg, REG_ROUNDINGS * EPS * max(rega, LD(reg_min)))
    eta = eta_from(a11, prev, eta_min, eta_max)
    out["eta"] = _ratio(sc[ETA], eta, 2 * EPS * eta)
    out["slot14"] = _exact(sc[GH_PREV], a11)
    regf = LD(sc[REG])
    dc = regf * si[:6 * C] ** 2
    out["Dc"] = _ratio(np.asarray(st["Dc"]).ravel(), dc, 2 * EPS * dc)
    P = np.asarray(V).shape[0]
    sp = si[6 * C:].reshape(P, 3)
    D = np.einsum("pi,ij->pij", regf * sp * sp, np.eye(3, dtype=LD))
    A = full_sym(np.asarray(V).astype(LD), 3) + D
    inv = eb._inv3(A)
    ai = np.abs(inv)
    bnd = (3 + eb.CHOL_ROUNDINGS) * EPS * np.einsum("pij,pjk,pkl->pil", ai, np.abs(A), ai)
    out["Vinv"] = _ratio(st["Vinv"], eb.upper(inv), eb.upper(bnd))
    if "e" not in skip and "e" in st:
        vf = full_sym(np.asarray(st["Vinv"]).astype(LD), 3)
        gl = np.asarray(gp).astype(LD)
        out["e"] = _ratio(st["e"], np.einsum("pij,pj->pi", vf, gl), 3 * EPS * np.einsum("pij,pj->pi", np.abs(vf), np.abs(gl)))
    if U is not None:
        Dcf = np.einsum("ci,ij->cij", np.asarray(st["Dc"]).astype(LD), np.eye(6, dtype=LD))
        M = full_sym(np.asarray(U).astype(LD), 6) + Dcf
        minv = eb._inv_spd(M)
        am = np.abs(minv)
        bnd = (1 + eb.SPD6_ROUNDINGS) * EPS * np.einsum("cij,cjk,ckl->cil", am, np.abs(M), am)
        out["Minv"] = _ratio(st["Minv"], eb.upper(minv), eb.upper(bnd))
    return out


# ---- step ----------------------------------------------------------------------------------------------------------------
def solve_tr_2d(B, g, Delta, T=LD, lam_shift=None):
    """min 0.5 p^T B p + g^T p, |p| <= Delta, B = (b11, b12, b22): the Newton step inside the region, else the boundary
    point from the secular equation in the eigenbasis of B (the global minimiser scipy's solve_trust_region_2d finds from
    its quartic) -> (p0, p1, lam or None).  lam_shift: the boundary solution at lam + lam_shift max(1, |lam|) -- what an
    iteration that stops that far from the root returns."""
    b11, b12, b22 = (T(v) for v in B)
    g0, g1, Delta = T(g[0]), T(g[1]), T(Delta)
    det = b11 * b22 - b12 * b12
    if b11 > 0 and det > 0:
        p0, p1 = -(b22 * g0 - b12 * g1) / det, -(-b12 * g0 + b11 * g1) / det
        if p0 * p0 + p1 * p1 <= Delta * Delta:
            return p0, p1, None
    if not Delta > 0:
        return T(0), T(0), None
    half, rad = T(0.5) * (b11 + b22), np.sqrt(T(0.25) * (b11 - b22) ** 2 + b12 * b12)
    l1, l2 = half - rad, half + rad
    if abs(b12) > 0:
        ax, ay, bx, by = b12, l1 - b11, l1 - b22, b12
        qx, qy = (ax, ay) if ax * ax + ay * ay >= bx * bx + by * by else (bx, by)
        nrm = np.sqrt(qx * qx + qy * qy)
        qx, qy = qx / nrm, qy / nrm
    else:
        qx, qy = (T(1), T(0)) if b11 <= b22 else (T(0), T(1))
    h1, h2 = qx * g0 + qy * g1, -qy * g0 + qx * g1
    gn = np.sqrt(h1 * h1 + h2 * h2)
    if gn == 0:
        return (Delta * qx, Delta * qy, None) if l1 < 0 else (T(0), T(0), None)
    lo, hi = max(T(0), -l1), gn / Delta - l1
    f = lambda lam: h1 * h1 / (l1 + lam) ** 2 + h2 * h2 / (l2 + lam) ** 2 - Delta * Delta
    if not f(lo) > 0:                                    # (the hard case: not met by a model with g along the first axis)
        raise ValueError("hard case of the 2-D trust-region problem")
    for _ in range(200):                                 # bisection to the last bit of the type
        mid = T(0.5) * (lo + hi)
        if mid <= lo or mid >= hi:
            break
        lo, hi = (mid, hi) if f(mid) > 0 else (lo, mid)
    lam = T(0.5) * (lo + hi)
    if lam_shift is not None:
        lam = lam + T(lam_shift) * max(T(1), abs(lam))
    c1, c2 = -h1 / (l1 + lam), -h2 / (l2 + lam)
    px, py = c1 * qx - c2 * qy, c1 * qy + c2 * qx
    nrm = np.sqrt(px * px + py * py)
    return px * Delta / nrm, py * Delta / nrm, lam


def tr_step(G, a, b, Delta, T=LD, lam_shift=None):
    """tr_build_model and tr_solve_step restated from ba_oracle.trf_schur (lines 534-562): G = (G11, G12, G22),
    a = (a11, a12, a22), b = (b11, b12, b22) -> (c1, c2, predicted, |step_h|, |step|)."""
    G11_, G12_, G22_ = (T(v) for v in G)
    a11, a12, a22 = (T(v) for v in a)
    b11, b12, b22 = (T(v) for v in b)
    s11 = np.sqrt(a11)
    r12 = a12 / s11
    r22sq = a22 - r12 * r12
    two_d = bool(r22sq > T(1e-28) * a22 and r22sq > 0)
    r22 = np.sqrt(r22sq) if two_d else T(1)
    if two_d:
        B = (G11_ / a11, (G12_ / s11 - r12 * G11_ / a11) / r22, (G22_ - 2 * r12 * G12_ / s11 + r12 * r12 * G11_ / a11) / (r22 * r22))
    else:
        B = (G11_ / a11, T(0), T(1))
    p0, p1, _ = solve_tr_2d(B, (s11, T(0)), Delta, T, lam_shift)
    if not two_d:
        p1 = T(0)
    pred = -(T(0.5) * (B[0] * p0 * p0 + 2 * B[1] * p0 * p1 + B[2] * p1 * p1) + s11 * p0)
    c2 = p1 / r22 if two_d else T(0)
    c1 = (p0 - (p1 * r12 / r22 if two_d else T(0))) / s11
    return np.array([c1, c2, pred, np.sqrt(p0 * p0 + p1 * p1), np.sqrt(max(T(0), c1 * c1 * b11 + 2 * c1 * c2 * b12 + c2 * c2 * b22))], dtype=T)


STEP_ROUNDINGS = 32
SECULAR_STOP = 1e-16         # tr2d.hpp: the secular iteration ends when lam moves by less than this times max(1, |lam|)


def model_inputs(sc):
    """(G11, G12, G22), (a11, a12, a22), (b11, b12, b22) from the scalars as k_tr_step and the host add them."""
    sc = np.asarray(sc)
    return ((sc[G11], sc[G12], sc[G22]), (qsum(sc, 1), qsum(sc, 5), qsum(sc, 6)), (qsum(sc, 4), qsum(sc, 7), qsum(sc, 8)))


def step_bound(G, a, b, Delta):
    """The five outputs and their bound.  The model and the 2x2 solve are a few dozen operations on ten scalars: each
    rounding is a relative perturbation of at most eps of one input (r12^2 <= a22 by Cauchy-Schwarz, so even the cancelling
    a22 - r12^2 is one of a22), hence the outputs are the exact outputs of inputs perturbed by STEP_ROUNDINGS eps
    (16 on the longest path of the model, B[2]; as many for the solve), to first order STEP_ROUNDINGS eps sum_i
    |d out / d in_i| |in_i|, with the derivatives by differences in longdouble; a boundary solution adds what a secular
    iteration stopped SECULAR_STOP max(1, lam) from its root moves the outputs by; and the outputs' own rounding."""
    ref = tr_step(G, a, b, Delta)
    h = LD(2.0) ** -24
    sens = np.zeros(5, dtype=LD)
    vals = list(G) + list(a) + list(b) + [Delta]
    for i in range(len(vals)):
        w = [LD(v) for v in vals]
        w[i] = w[i] * (1 + h)
        sens += np.abs(tr_step(w[0:3], w[3:6], w[6:9], w[9]) - ref) / h
    stop = np.abs(tr_step(G, a, b, Delta, lam_shift=SECULAR_STOP) - ref) + np.abs(tr_step(G, a, b, Delta, lam_shift=-SECULAR_STOP) - ref)
    return ref, STEP_ROUNDINGS * EPS * (sens + np.abs(ref)) + stop


def check_step(sc):
    """k_tr_step from the fetched scalars (step_bound); the skip flag is down."""
    sc = np.asarray(sc)
    G, a, b = model_inputs(sc)
    ref, bnd = step_bound(G, a, b, sc[RADIUS])
    out = {name: _ratio(sc[STEP + k], ref[k], bnd[k]) for k, name in enumerate(("c1", "c2", "predicted", "step_h", "step"))}
    out["skip"] = _exact(sc[SKIP], 0.0)
    return out


def check_x_new(x_new, x, sg, p, c1, c2):
    """k_step_table from the fetched vectors: x_new = x + c1 sg + c2 p, two products and two additions, within 3 eps of
    the summed magnitudes."""
    xl, sgl, pl, c1, c2 = np.asarray(x).astype(LD), np.asarray(sg).astype(LD), np.asarray(p).astype(LD), LD(c1), LD(c2)
    return {"x_new": _ratio(x_new, xl + c1 * sgl + c2 * pl, 3 * EPS * (np.abs(xl) + np.abs(c1 * sgl) + np.abs(c2 * pl)))}


# ---- pcg -----------------------------------------------------------------------------------------------------------------
class SchurSystem:
    """S = U + diag(Dc) - W (V + diag(dp))^-1 W^T and b = -g_c + sum W (V + diag dp)^-1 g_p from the blocks r (N, 2),
    Jc (N, 2, 6), Jp (N, 2, 3), in the blocks' own precision (float64: numpy's sums; longdouble: entry_bounds'
    Linearisation).  The camera blocks of held cameras' observations are zeroed (ba_oracle.trf_schur)."""

    def __init__(self, r, Jc, Jp, ci, pi, C, P, Dc, dp, held=(), dp_in_vinv=True, dc_in_w=True, fetched=None):
        T = Jc.dtype.type
        self.T, self.C, self.P, self.ci, self.pi = T, C, P, np.asarray(ci), np.asarray(pi)
        Jc = Jc.copy()
        if len(held):
            Jc[np.isin(self.ci, np.asarray(list(held), dtype=np.int64))] = 0
        self.Jc, self.Jp = Jc, Jp
        self.Dc = np.asarray(Dc).reshape(C, 6).astype(T)
        self.dc_in_w = dc_in_w
        V, self.gp, self.gc = np.zeros((P, 3, 3), dtype=T), np.zeros((P, 3), dtype=T), np.zeros((C, 6), dtype=T)
        np.add.at(V, self.pi, np.einsum("nki,nkj->nij", Jp, Jp))
        np.add.at(self.gp, self.pi, np.einsum("nki,nk->ni", Jp, r))
        np.add.at(self.gc, self.ci, np.einsum("nki,nk->ni", Jc, r))
        if dp_in_vinv:
            V = V + np.einsum("pi,ij->pij", np.asarray(dp).reshape(P, 3).astype(T), np.eye(3, dtype=T))
        self.Vinv = eb._inv3(V)
        self.U = np.zeros((C, 6, 6), dtype=T)
        np.add.at(self.U, self.ci, np.einsum("nki,nkj->nij", Jc, Jc))
        if fetched is not None:                          # g_c (C, 6), g_p (P, 3) and the packed Vinv (P, 6) as a device left them
            self.gc, self.gp = np.asarray(fetched["gc"]).astype(T), np.asarray(fetched["gp"]).astype(T)
            self.Vinv = full_sym(np.asarray(fetched["Vinv"]).astype(T), 3)

    def _to_cams(self, per_obs):
        out = np.zeros((self.C, 6), dtype=self.T)
        np.add.at(out, self.ci, np.einsum("nki,nk->ni", self.Jc, per_obs))
        return out

    def rhs(self):
        e = np.einsum("pij,pj->pi", self.Vinv, self.gp)
        return -self.gc + self._to_cams(np.einsum("nki,ni->nk", self.Jp, e[self.pi]))

    def mv(self, v):
        v = v.reshape(self.C, 6)
        t = np.einsum("nki,ni->nk", self.Jc, v[self.ci])
        y = np.zeros((self.P, 3), dtype=self.T)
        np.add.at(y, self.pi, np.einsum("nki,nk->ni", self.Jp, t))
        z = np.einsum("pij,pj->pi", self.Vinv, y)
        out = self._to_cams(t - np.einsum("nki,ni->nk", self.Jp, z[self.pi]))
        return out + self.Dc * v if self.dc_in_w else out

    def back_substitute(self, dc):
        t = np.einsum("nki,ni->nk", self.Jc, dc.reshape(self.C, 6)[self.ci])
        y = np.zeros((self.P, 3), dtype=self.T)
        np.add.at(y, self.pi, np.einsum("nki,nk->ni", self.Jp, t))
        return np.einsum("pij,pj->pi", self.Vinv, -self.gp - y)

    def diagonal_blocks(self, exact_pairs):
        """The diagonal 6x6 blocks of S: one term W Vinv W^T per observation (k_cam_rhs_diag), or (exact_pairs) the blocks of
        the formed S, in which several observations of one camera and point also contribute their cross terms (k_schur_blocks)."""
        W = np.einsum("nki,nkj->nij", self.Jc, self.Jp)
        ci, pi = self.ci, self.pi
        if exact_pairs:
            uniq, inv = np.unique(ci.astype(np.int64) * self.P + pi, return_inverse=True)
            Ws = np.zeros((len(uniq), 6, 3), dtype=self.T)
            np.add.at(Ws, inv, W)
            W, ci, pi = Ws, uniq // self.P, uniq % self.P
        Sd = self.U + np.einsum("ci,ij->cij", self.Dc, np.eye(6, dtype=self.T))
        np.add.at(Sd, ci, -np.einsum("nik,nkl,njl->nij", W, self.Vinv[pi], W))
        return Sd


def pcg(system, Minv, iters=None, tol2=None, max_iters=None, beta_wrong_gamma=False):
    """Textbook block-preconditioned CG on S x = b from x = 0: exactly `iters` iterations, or (iters = None) until
    rz <= tol2 rz0.  -> x, r (C, 6), [rz_0 .. rz_k].  beta_wrong_gamma: the planted error -- beta from the gamma before
    the previous one."""
    T = system.T
    Minv = np.asarray(Minv).astype(T)
    b = system.rhs()
    x, r = np.zeros_like(b), b.copy()
    z = np.einsum("cij,cj->ci", Minv, r)
    p = z.copy()
    rz = [np.sum(r * z)]
    k = 0
    while (k < iters) if iters is not None else (rz[-1] > tol2 * rz[0] and k < max_iters):
        if not rz[-1] > 0:
            break
        Ap = system.mv(p)
        alpha = rz[-1] / np.sum(p * Ap)
        x, r = x + alpha * p, r - alpha * Ap
        z = np.einsum("cij,cj->ci", Minv, r)
        rz.append(np.sum(r * z))
        den = rz[-3] if beta_wrong_gamma and len(rz) >= 3 else rz[-2]
        p = z + (rz[-1] / den) * p
        k += 1
    return x, r, rz, b


def block_rel(err, ref):
    """Largest  |err_c|_inf / |ref_c|_inf  over the camera blocks; a block whose reference is zero has to be zero."""
    e, m = np.abs(np.asarray(err, dtype=LD)).max(axis=1), np.abs(np.asarray(ref, dtype=LD)).max(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(m > 0, e / m, np.where(e == 0, 0.0, np.inf))
    return float(q.max())


def pcg_measures(sys_ld, x, r, rz, ref):
    """The three figures the golden file records and the GPU test is held to: dc by camera block, the residual identity
    r + S x - b by camera block (against b), and the relative error of rz0 and of the last rz."""
    xl, rl, rzl, bl = ref
    ident = np.asarray(r).astype(LD) + sys_ld.mv(np.asarray(x).astype(LD)) - bl if r is not None else None
    return {"dc": block_rel(np.asarray(x).astype(LD) - xl, xl),
            "identity": block_rel(ident, bl) if ident is not None else None,
            "rz": float(max(abs(LD(rz[0]) - rzl[0]) / rzl[0], abs(LD(rz[-1]) - rzl[-1]) / rzl[-1]))}


def check_identity(case, sys_ld, st):
    """The residual identity alone, on an operator built from fetched blocks: r + S x - b by camera block against b, within
    factor x the case's recorded figure."""
    bounds = load_bounds()
    b = sys_ld.rhs()
    ident = np.asarray(st["pcg_r"]).astype(LD) + sys_ld.mv(np.asarray(st["pcg_x"]).astype(LD)) - b
    return {"identity": block_rel(ident, b) / (bounds["factor"] * bounds["cases"][case]["identity"])}


def load_bounds():
    with open(BOUNDS_FILE) as f:
        return json.load(f)


def check_pcg(case, lin, st, ctrl, sc, C, P, held=(), dense=False, pcg_tol=None, minv=None):
    """The PCG from x (lin: its longdouble linearisation), the fetched Dc, reg si_p^2, Minv and ctrl.iters: exactly that
    many textbook iterations in longdouble.  dc, the residual identity and rz within factor x what the reference's own two
    precisions differ by (iteration_bounds.json); the stop rule in the reference and on the device; tol2's own bits."""
    bounds = load_bounds()
    rec, factor = bounds["cases"][case], bounds["factor"]
    si = np.asarray(st["si"])
    dp = (sc[REG] * si[6 * C:]) * si[6 * C:]
    sys_ld = SchurSystem(lin.r, lin.Jc, lin.Jp, lin.ci, lin.pi, C, P, st["Dc"], dp, held)
    Minv = eb._inv_spd(sys_ld.diagonal_blocks(True)) if dense else full_sym(np.asarray(st["Minv"] if minv is None else minv).astype(LD), 6)
    iters = ctrl["iters"]
    ref = pcg(sys_ld, Minv, iters=iters)
    rzl = ref[2]
    dc = np.asarray(st["p"])[:6 * C].reshape(C, 6)
    m = pcg_measures(sys_ld, dc, st.get("pcg_r"), (ctrl["rz0"], ctrl["rz"]), ref)
    out = {"dc": m["dc"] / (factor * rec["dc"]), "rz": m["rz"] / (factor * rec["rz"])}
    if m["identity"] is not None:
        out["identity"] = m["identity"] / (factor * rec["identity"])
    if "pcg_x" in st:
        out["pcg_x_is_dc"] = _exact(st["pcg_x"], dc)
    tol = DENSE_TOL_FACTOR * pcg_tol if dense else sc[ETA]
    out["tol2"] = _exact(ctrl["tol2"], tol * tol)
    t2 = LD(ctrl["tol2"])
    ok = iters >= 1 and len(rzl) == iters + 1 and rzl[iters] <= t2 * rzl[0] and all(rzl[k] > t2 * rzl[0] for k in range(1, iters))
    out["stop_rule_reference"] = 0.0 if ok else math.inf
    ok = ctrl["done"] == 1 and ctrl["rz"] <= ctrl["tol2"] * ctrl["rz0"] and (iters == 1 or ctrl["rz_prev"] > ctrl["tol2"] * ctrl["rz0"])
    out["stop_rule_device"] = 0.0 if ok else math.inf
    out["iters_recorded"] = _exact(iters, rec["iters"])
    return out


# ---- the iteration in plain float64 -----------------------------------------------------------------------------------------
def _slice_sums(sc, si, g, sg, x, C):
    for sl, slot in ((slice(0, 6 * C), lambda q: CAM_SLOT + q), (slice(6 * C, None), lambda q: POINT_SLOT[q])):
        sc[slot(0)] = np.abs(g[sl]).max() if len(g[sl]) else 0.0
        sc[slot(1)], sc[slot(2)] = np.sum((g[sl] / si[sl]) ** 2), np.sum((x[sl] * si[sl]) ** 2)
        sc[slot(3)], sc[slot(4)] = np.sum(x[sl] ** 2), np.sum(sg[sl] ** 2)


def replay(orc, args, x, si_old=None, prev=0.0, Delta=None, held=(), precond=True, dense=False, plant=None,
           pcg_tol=1e-2, pcg_tol_max=0.1, reg_min=1e-6, iters=None):
    """One outer iteration at x in float64 -> (state in the layout of Backend.iteration_state plus U, V, gc, gp, pcg_r, e,
    `system` and the PCG's rz list).  si_old / prev / Delta: None / 0 / None at the start of a solve.  `plant`: one of
    PLANTS.  `iters`: run exactly that many PCG iterations instead of the stop rule."""
    C, P, ci, pi, uv, K = args
    ci, pi = np.asarray(ci), np.asarray(pi)
    x = np.asarray(x, dtype=np.float64)
    r, Jc, Jp = orc.jacobian_blocks(x, *args)
    hmask = np.isin(ci, np.asarray(list(held), dtype=np.int64))
    Jcz = Jc.copy()
    Jcz[hmask] = 0.0
    nb = orc.normal_blocks(r, Jcz, Jp, C, P, ci, pi)
    U, V, gc, gp = eb.upper(nb.U), eb.upper(nb.V), nb.gc, nb.gp
    d = np.concatenate([U[:, DIAG_U].ravel(), V[:, DIAG_V].ravel()])
    if plant == "held_scale_not_one" and len(held):      # the scale from the blocks the held cameras would have had
        d[:6 * C] = np.einsum("cii->ci", orc.normal_blocks(r, Jc, Jp, C, P, ci, pi).U).ravel()
    si = np.sqrt(d)
    if si_old is None:
        si[d == 0] = 1.0
    elif plant != "scale_forgets_max":
        si = np.maximum(si, si_old)
    else:
        si[si == 0] = 1.0
    g = np.concatenate([gc.ravel(), gp.ravel()])
    sg = g / (si * si)
    sc = np.zeros(32)
    sc[0] = np.sum(r * r)
    _slice_sums(sc, si, g, sg, x, C)
    jdot = lambda v: np.einsum("nki,ni->nk", Jcz, v[:6 * C].reshape(C, 6)[ci]) + np.einsum("nki,ni->nk", Jp, v[6 * C:].reshape(P, 3)[pi])
    t1 = jdot(sg)
    sc[G11] = np.sum(t1 * t1)
    a11 = sc[8] + sc[CAM_SLOT + 1]
    if Delta is None:
        d2 = sc[9] + sc[CAM_SLOT + 2]
        Delta = math.sqrt(d2) if d2 != 0 else 1.0
    sc[RADIUS] = Delta
    sc[REG] = float(reg_from_scalars(a11, sc[G11], Delta, reg_min, T=np.float64)[0])
    eta_min, eta_max = pcg_tol, max(pcg_tol, pcg_tol_max)
    sc[ETA] = float(eta_from(a11, prev, eta_min, eta_max, T=np.float64))
    if plant == "eta_never_clamped" and prev > 0:
        sc[ETA] = math.sqrt(a11 / prev)
    sc[GH_PREV] = a11
    Dc = ((sc[REG] * si[:6 * C]) * si[:6 * C]).reshape(C, 6)
    dp = (sc[REG] * si[6 * C:]) * si[6 * C:]
    system = SchurSystem(r, Jc, Jp, ci, pi, C, P, Dc, dp, held, dp_in_vinv=plant != "dp_missing_from_vinv",
                         dc_in_w=plant != "dc_missing_from_w")
    if precond:
        Minv = np.linalg.inv(system.diagonal_blocks(dense))
    else:
        Minv = np.linalg.inv(nb.U + np.einsum("ci,ij->cij", Dc, np.eye(6)))
    tol = DENSE_TOL_FACTOR * pcg_tol if dense else sc[ETA]
    xk, rk, rz, _ = pcg(system, Minv, iters=iters, tol2=tol * tol, max_iters=max(20, 12 * C), beta_wrong_gamma=plant == "beta_wrong_gamma")
    dpt = system.back_substitute(xk)
    p = np.concatenate([xk.ravel(), dpt.ravel()])
    t2 = jdot(p)
    sc[G12], sc[G22] = np.sum(t1 * t2), np.sum(t2 * t2)
    for sl, slot in ((slice(0, 6 * C), lambda q: CAM_SLOT + q), (slice(6 * C, None), lambda q: POINT_SLOT[q])):
        sc[slot(5)], sc[slot(6)] = np.sum(g[sl] * p[sl]), np.sum((p[sl] * si[sl]) ** 2)
        sc[slot(7)], sc[slot(8)] = np.sum(sg[sl] * p[sl]), np.sum(p[sl] ** 2)
    G, a, b = model_inputs(sc)
    sc[STEP:STEP + 5] = tr_step(G, a, b, Delta, T=np.float64).astype(np.float64)
    x_new = x + sc[STEP] * sg + sc[STEP + 1] * p
    ctrl = {"rz": float(rz[-1]), "rz0": float(rz[0]), "tol2": tol * tol, "rz_prev": float(rz[-2]) if len(rz) > 1 else 1.0,
            "alpha_prev": 1.0, "iters": len(rz) - 1, "max_iters": max(20, 12 * C), "done": 1 if rz[-1] <= tol * tol * rz[0] else 2}
    return {"scalars": sc, "ctrl": ctrl, "si": si, "g": g, "sg": sg, "Dc": Dc, "Minv": eb.upper(Minv), "Vinv": eb.upper(system.Vinv),
            "e": np.einsum("pij,pj->pi", system.Vinv, gp), "pcg_x": xk, "pcg_r": rk, "p": p, "x_new": x_new, "U": U, "V": V, "gc": gc, "gp": gp,
            "x": x, "rz": rz, "system": system, "model": (G, a, b)}


def update_radius(Delta, actual, predicted, step_h_norm):
    """update_tr_radius of scipy's common.py as ba_oracle.trf_schur restates it -> (Delta, ratio)."""
    ratio = actual / predicted if predicted > 0 else (1.0 if predicted == actual == 0 else 0.0)
    if ratio < 0.25:
        return 0.25 * step_h_norm, ratio
    if ratio > 0.75 and step_h_norm > 0.95 * Delta:
        return 2.0 * Delta, ratio
    return Delta, ratio


def trf(orc, args, x0, plant=None, held=(), ftol=1e-8, xtol=1e-8, gtol=1e-8, max_nfev=None, **kw):
    """ba_oracle.trf_schur's outer loop over `replay`: the old standard's view of a (planted) iteration -- status, nfev,
    njev, cost, x -- and the replayed state of every outer iteration (`states`; `inputs`: si_old, prev, Delta of each)."""
    x = np.asarray(x0, dtype=np.float64).copy()
    n = len(x)
    max_nfev = 100 * n if max_nfev is None else max_nfev
    si_old, prev, Delta, cost, status = None, 0.0, None, None, None
    nfev = njev = 1
    states, inputs = [], []
    while True:
        it = replay(orc, args, x, si_old, prev, Delta, held, plant=plant, **kw)
        sc = it["scalars"]
        if cost is None:
            cost = 0.5 * sc[0]
        inputs.append({"si_old": si_old, "prev": prev, "Delta": Delta})
        states.append(it)
        Delta = sc[RADIUS]
        if max(sc[POINT_SLOT[0]], sc[CAM_SLOT]) < gtol:
            status = 1
        if status is not None or nfev >= max_nfev:
            break
        G, a, b = it["model"]
        x_norm = math.sqrt(qsum(sc, 3))
        actual, first, x_new, cost_new = -1.0, True, x, cost
        while actual <= 0 and nfev < max_nfev:
            stp = sc[STEP:STEP + 5] if first else tr_step(G, a, b, Delta, T=np.float64)
            first = False
            x_new = x + stp[0] * it["sg"] + stp[1] * it["p"]
            cost_new = 0.5 * float(np.sum(orc.compute_residuals(x_new, *args) ** 2))
            nfev += 1
            if not np.isfinite(cost_new):
                Delta = 0.25 * stp[3]
                continue
            actual = cost - cost_new
            Delta_new, ratio = update_radius(Delta, actual, stp[2], stp[3])
            f_ok, x_ok = actual < ftol * cost and ratio > 0.25, stp[4] < xtol * (xtol + x_norm)
            status = 4 if f_ok and x_ok else 2 if f_ok else 3 if x_ok else None
            if status is not None:
                break
            Delta = Delta_new
        si_old, prev = it["si"], sc[GH_PREV]
        if actual > 0:
            x, cost = x_new, cost_new
            njev += 1
        if status is not None:
            break
    return {"status": 0 if status is None else status, "nfev": nfev, "njev": njev, "cost": cost, "x": x, "states": states, "inputs": inputs}


# ---- the PCG cases whose bounds tools/gen_iteration_golden.py measures ---------------------------------------------------------
# name -> problem, held cameras, Schur-diagonal preconditioner, dense path, outer iteration
PCG_CASES = {
    "hand_built": dict(problem="hand_built", held=(), precond=True, dense=False, iteration=0),
    "hand_built_precond0": dict(problem="hand_built", held=(), precond=False, dense=False, iteration=0),
    "schur_1024": dict(problem="schur_1024", held=(), precond=True, dense=False, iteration=0),
    "schur_1025": dict(problem="schur_1025", held=(), precond=True, dense=False, iteration=0),
    "dense_21": dict(problem="dense_%d" % eb.DENSE_CAMERAS, held=(), precond=True, dense=True, iteration=0),
    "held": dict(problem="held", held=(0, 9), precond=True, dense=False, iteration=0),
}
MARGIN = 1e-6                # rz / (tol2 rz0) at iters and at iters - 1 stays this far from 1 in the longdouble replay


def case_problem(name, orc):
    """-> (args, x0) of a problem of PCG_CASES / of the GPU test's table."""
    import sfmba
    if name == "held":
        pb = sfmba.make_problem(15, 200, 1500)
    elif name == "running_max":
        pb = sfmba.make_problem(6, 80, 500, seed=1)
    elif name == "far_start":
        pb = sfmba.make_problem(6, 80, 500, seed=5, x0_noise=0.2)
    else:
        return eb.problem(name, orc)
    return pb.args, pb.x0


def measure_pcg_case(name, orc):
    """One case of the golden file: the float64 replay's operands, the PCG in longdouble to its stop rule (iters), the
    same number of iterations in float64, and what the two differ by."""
    case = PCG_CASES[name]
    args, x0 = case_problem(case["problem"], orc)
    C, P = args[0], args[1]
    st = replay(orc, args, x0, held=case["held"], precond=case["precond"], dense=case["dense"])
    sc = st["scalars"]
    lin = eb.Linearisation(*args, x0)
    si = st["si"]
    dp = (sc[REG] * si[6 * C:]) * si[6 * C:]
    sys_ld = SchurSystem(lin.r, lin.Jc, lin.Jp, lin.ci, lin.pi, C, P, st["Dc"], dp, case["held"])
    Minv = full_sym(st["Minv"], 6)
    tol2 = LD(st["ctrl"]["tol2"])
    # (the dense path keeps its inverse blocks in LDS: there each precision inverts the diagonal blocks of its own S, as
    # check_pcg's reference has to)
    ref = pcg(sys_ld, eb._inv_spd(sys_ld.diagonal_blocks(True)) if case["dense"] else Minv.astype(LD), tol2=tol2, max_iters=st["ctrl"]["max_iters"])
    rzl = ref[2]
    iters = len(rzl) - 1
    x64, r64, rz64, _ = pcg(st["system"], Minv, iters=iters)
    m = pcg_measures(sys_ld, x64, r64, rz64, ref)
    return dict(m, iters=iters, done=1 if rzl[-1] <= tol2 * rzl[0] else 2, margin_at=float(rzl[iters] / (tol2 * rzl[0])),
                margin_before=float(rzl[iters - 1] / (tol2 * rzl[0])) if iters >= 1 else None)
