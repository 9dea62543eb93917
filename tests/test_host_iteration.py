"""The layer checks of tests/iteration_ref.py without a GPU: the float64 replay of an outer iteration lies inside every
bound the GPU test holds the device to; the two conditions on the PCG cases hold; and each of six subtly wrong
iterations is rejected by a named check while the whole-solve standard -- status, nfev, njev equal, cost within 1e-8 --
accepts it on the same problem.  The planted iterations run through ba_oracle.trf_schur's loop as iteration_ref.trf
restates it over `replay` (the unplanted loop reproduces the oracle's counts and cost, asserted below)."""
import warnings

import numpy as np
import pytest

import entry_bounds as eb
import iteration_ref as ir

pytestmark = pytest.mark.skipif(not eb.extended_precision(), reason="numpy.longdouble is no wider than a double on this machine")


@pytest.fixture(scope="module")
def orc():
    from oracle import ba_oracle
    return ba_oracle


def _inside(tag, layer, out):
    print(f"{tag} {layer}: worst error / bound {max(out.values()):.3g}")
    bad = {k: v for k, v in out.items() if not v <= 1.0}
    assert not bad, (tag, layer, bad)


def _layer_checks(st, inp, C, held=(), precond=True):
    """Every counted layer on a replayed state -> {layer: {check: error / bound}}."""
    sc, x = st["scalars"], st["x"]
    first = inp["si_old"] is None
    return {"scale": ir.check_scale(st, st["U"], st["V"], st["gc"], st["gp"], x, C, si_old=inp["si_old"], held=held),
            "sums": ir.check_scale_sums(sc, st, x, C),
            "prep": ir.check_prep(sc, st, st["V"], st["gp"], C, 1e-6, 1e-2, 0.1, prev=inp["prev"], first=first, U=None if precond else st["U"]),
            "step": ir.check_step(sc),
            "x_new": ir.check_x_new(st["x_new"], x, st["sg"], st["p"], sc[ir.STEP], sc[ir.STEP + 1])}


START = {"si_old": None, "prev": 0.0, "Delta": None}


# ---- the float64 replay inside every bound ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ir.PCG_CASES))
def test_float64_replay_lies_inside_every_bound(orc, name):
    case = ir.PCG_CASES[name]
    args, x0 = ir.case_problem(case["problem"], orc)
    C, P = args[0], args[1]
    st = ir.replay(orc, args, x0, held=case["held"], precond=case["precond"], dense=case["dense"])
    for layer, out in _layer_checks(st, START, C, case["held"], case["precond"]).items():
        _inside(name, layer, out)
    lin = eb.Linearisation(*args, x0)
    _inside(name, "pcg", ir.check_pcg(name, lin, st, st["ctrl"], st["scalars"], C, P, held=case["held"], dense=case["dense"], pcg_tol=1e-2))


def test_float64_replay_of_later_iterations(orc):
    """Iterations 1 and 2 of the running-maximum problem: the scale's maximum holds entries, eta adapts and is clamped."""
    args, x0 = ir.case_problem("running_max", orc)
    run = ir.trf(orc, args, x0, max_nfev=4)
    etas = [float(s["scalars"][ir.ETA]) for s in run["states"]]
    assert 1e-2 < etas[1] < 0.1 and etas[2] == 0.1, etas
    d = np.concatenate([run["states"][1]["U"][:, ir.DIAG_U].ravel(), run["states"][1]["V"][:, ir.DIAG_V].ravel()])
    assert (run["states"][0]["si"] > np.sqrt(d) * (1 + 4 * ir.EPS)).any()
    for k in (1, 2):
        for layer, out in _layer_checks(run["states"][k], run["inputs"][k], args[0]).items():
            _inside(f"running_max[{k}]", layer, out)


def test_restated_loop_reproduces_the_oracle(orc):
    for problem, held in (("running_max", ()), ("far_start", ()), ("held", (0, 9))):
        args, x0 = ir.case_problem(problem, orc)
        mine = ir.trf(orc, args, x0, held=held, ftol=1e-10)
        o = orc.trf_schur(x0, *args, ftol=1e-10, linear="pcg", pcg_tol=1e-2, pcg_tol_max=0.1, precond="schur", fixed_cameras=held)
        assert (mine["status"], mine["nfev"], mine["njev"]) == (o.status, o.nfev, o.njev), problem
        assert abs(mine["cost"] - o.cost) <= 1e-9 * o.cost, problem


def test_step_reference_agrees_with_the_oracles_quartic(orc):
    """tr_step (the secular form) against ba_oracle.solve_trust_region_2d (scipy's quartic) on a model with a boundary
    solution and on one with the Newton step inside."""
    args, x0 = ir.case_problem("running_max", orc)
    G, a, b = ir.replay(orc, args, x0)["model"]
    s11 = np.sqrt(a[0])
    r12 = a[1] / s11
    r22 = np.sqrt(a[2] - r12 * r12)
    B = np.array([[G[0] / a[0], (G[1] / s11 - r12 * G[0] / a[0]) / r22], [0.0, (G[2] - 2 * r12 * G[1] / s11 + r12 * r12 * G[0] / a[0]) / (r22 * r22)]])
    B[1, 0] = B[0, 1]
    newton = -np.linalg.solve(B, [s11, 0.0])
    for Delta, inside in ((0.01 * np.linalg.norm(newton), False), (2.0 * np.linalg.norm(newton), True)):
        pS, took = orc.solve_trust_region_2d(B, np.array([s11, 0.0]), Delta)
        assert took == inside
        ref = ir.tr_step(G, a, b, Delta)
        c2 = pS[1] / r22
        c1 = (pS[0] - pS[1] * r12 / r22) / s11
        assert abs(float(ref[0]) - c1) <= 1e-9 * abs(c1) and abs(float(ref[1]) - c2) <= 1e-9 * abs(c2), (Delta, ref[:2], c1, c2)
        assert abs(float(ref[3]) - np.linalg.norm(pS)) <= 1e-12 * np.linalg.norm(pS)


# ---- the conditions on the PCG cases ---------------------------------------------------------------------------------------------
def test_golden_pcg_cases_meet_their_conditions(orc):
    bounds = ir.load_bounds()
    assert bounds["factor"] == 100.0 and set(bounds["cases"]) == set(ir.PCG_CASES)
    for name, rec in bounds["cases"].items():
        m = ir.measure_pcg_case(name, orc)
        assert m["iters"] == rec["iters"] and m["done"] == rec["done"] == 1, (name, m, rec)          # never a breakdown, never the cap
        for k in ("margin_at", "margin_before"):
            assert abs(m[k] - 1.0) >= ir.MARGIN and abs(rec[k] - 1.0) >= ir.MARGIN, (name, k, m[k])
        assert m["margin_at"] < 1.0 < m["margin_before"], (name, m)
        for k in ("dc", "identity", "rz"):               # numpy's sums may differ from the generating machine's: far inside the factor
            assert rec[k] > 0 and m[k] <= 10.0 * rec[k], (name, k, m[k], rec[k])


# ---- six planted errors ------------------------------------------------------------------------------------------------------------
def _pcg_ratio(orc, st, args, held=()):
    """The PCG layer on any replayed state: the state's dc, residual identity and rz against the longdouble PCG on the
    state's own operands, in units of factor x what an honest float64 PCG on them is off by."""
    C, P = args[0], args[1]
    sc, si = st["scalars"], st["si"]
    lin = eb.Linearisation(*args, st["x"])
    dp = (sc[ir.REG] * si[6 * C:]) * si[6 * C:]
    sys_ld = ir.SchurSystem(lin.r, lin.Jc, lin.Jp, lin.ci, lin.pi, C, P, st["Dc"], dp, held)
    Minv, iters = ir.full_sym(st["Minv"], 6), st["ctrl"]["iters"]
    ref = ir.pcg(sys_ld, Minv.astype(ir.LD), iters=iters)
    r, Jc, Jp = orc.jacobian_blocks(st["x"], *args)
    honest = ir.pcg(ir.SchurSystem(r, Jc, Jp, args[2], args[3], C, P, st["Dc"], dp, held), Minv, iters=iters)
    h = ir.pcg_measures(sys_ld, honest[0], honest[1], honest[2], ref)
    m = ir.pcg_measures(sys_ld, st["pcg_x"], st["pcg_r"], st["rz"], ref)
    return {k: m[k] / (100.0 * h[k]) for k in ("dc", "identity", "rz")}


def _plant_problem(orc):
    import sfmba
    pb = sfmba.make_problem(6, 40, 500, seed=1)
    return pb.args, pb.x0


# plant -> (problem, held, which check of which layer rejects it)
PLANTED = {
    "beta_wrong_gamma": ("running_max", (), ("pcg", "dc")),
    "dc_missing_from_w": ("plant", (), ("pcg", "identity")),
    "scale_forgets_max": ("running_max", (), ("scale", "si")),
    "eta_never_clamped": ("running_max", (), ("prep", "eta")),
    "dp_missing_from_vinv": ("plant", (), ("prep", "Vinv")),
    "held_scale_not_one": ("held", (0, 9), ("scale", "held")),
}


def _run(orc, problem, held, plant, **kw):
    args, x0 = _plant_problem(orc) if problem == "plant" else ir.case_problem(problem, orc)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                   # (a planted iteration may divide by zero)
        return args, ir.trf(orc, args, x0, plant=plant, held=held, ftol=1e-10, **kw)


def _old_standard_accepts(base, run):
    return ((run["status"], run["nfev"], run["njev"]) == (base["status"], base["nfev"], base["njev"])
            and abs(run["cost"] - base["cost"]) <= 1e-8 * base["cost"])


@pytest.mark.parametrize("plant", list(ir.PLANTS))
def test_planted_error_is_rejected_by_a_named_check_and_accepted_by_the_old_standard(orc, plant):
    problem, held, (layer, check) = PLANTED[plant]
    args, base = _run(orc, problem, held, None)
    _, run = _run(orc, problem, held, plant)
    C = args[0]
    worst_honest, worst_planted = 0.0, 0.0
    for states, label in ((base["states"], "honest"), (run["states"], "planted")):
        worst = 0.0
        for k, st in enumerate(states):
            inp = (base if label == "honest" else run)["inputs"][k]
            if layer == "pcg":
                if st["ctrl"]["iters"] < 3:
                    continue                              # (beta enters p after two iterations)
                out = _pcg_ratio(orc, st, args, held)
            else:
                out = _layer_checks(st, inp, C, held)[layer]
            worst = max(worst, out[check])
        if label == "honest":
            worst_honest = worst
        else:
            worst_planted = worst
    accepted = _old_standard_accepts(base, run)
    print(f"{plant}: {layer}.{check} error / bound honest {worst_honest:.3g}, planted {worst_planted:.3g}; whole-solve standard: "
          f"status {run['status']} nfev {run['nfev']} njev {run['njev']} cost off by {abs(run['cost'] - base['cost']) / base['cost']:.2e} "
          f"-> {'accepts' if accepted else 'CATCHES'} it (x off by {np.abs(run['x'] - base['x']).max():.2e})")
    assert worst_honest <= 1.0, (plant, worst_honest)
    assert worst_planted > 1.0, (plant, worst_planted)
    assert accepted, plant


def test_plants_the_old_standard_does_catch(orc):
    """No single small problem lets all five through: on make_problem(6, 80, 500, seed=1) a Dc missing from w ends the solve
    one evaluation earlier and a dp left out of Vinv meets rank-deficient point blocks; on make_problem(6, 40, 500, seed=1)
    a scale without its maximum and an unclamped eta change the status the solve ends with.  Reported, not dropped: each
    plant above is shown on the problem that lets it through."""
    plants = ("beta_wrong_gamma", "dc_missing_from_w", "scale_forgets_max", "eta_never_clamped", "dp_missing_from_vinv")
    verdict = {}
    for problem in ("running_max", "plant"):
        _, base = _run(orc, problem, (), None)
        for plant in plants:
            _, run = _run(orc, problem, (), plant, max_nfev=40)
            verdict[problem, plant] = _old_standard_accepts(base, run)
            print(f"{problem} {plant}: status {run['status']} nfev {run['nfev']} njev {run['njev']} (honest {base['status']} {base['nfev']} "
                  f"{base['njev']}) -> {'accepted' if verdict[problem, plant] else 'caught'}")
    caught = {k for k, v in verdict.items() if not v}
    assert caught == {("running_max", "dc_missing_from_w"), ("running_max", "dp_missing_from_vinv"), ("plant", "scale_forgets_max"),
                      ("plant", "eta_never_clamped")}, caught
