"""One outer iteration layer by layer, from what it leaves on the handle (tests/iteration_ref.py has the references, the
counts and the contract; DESIGN.md section 20, "The layers of an outer iteration").  A solve with max_nfev = 1 runs the
linear phase and the device-decided trial of iteration 0; `Backend.iteration_state()` fetches what they left, and every
layer -- scale, prep, pcg, step -- is checked from the fetched output of the layer before it.  One rank (but for the
world of one), 64-bit storage unless noted, every case a Backend of its own with its form asserted.  Every line
`iteration: <case> <layer> worst error / bound ...` of the output is a recorded value of profiles/iteration_gpu.txt."""
import os
import time

import numpy as np
import pytest

import entry_bounds as eb
import iteration_ref as ir
from conftest import ROOT

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not eb.extended_precision(), reason="numpy.longdouble is no wider than a double on this machine")]

LOCAL = dict(one_rank=1, dense_solve=0, precond=1, pcg_fused=1, pcg_local=1, pcg_split=0, quick_start=1, spec_scale=1, cost_rider=1)


@pytest.fixture(scope="module")
def orc():
    from oracle import ba_oracle
    return ba_oracle


@pytest.fixture(scope="module", autouse=True)
def wall_time():
    t0 = time.time()
    yield
    print(f"\niteration: wall time of the module {time.time() - t0:.1f} s")


@pytest.fixture
def opened():
    """opened(options, bits = 64, fixed = ()) -> a Backend of its own with these debug options; closed when the test ends."""
    import sfmba
    made = []

    def open_(options, bits=64, fixed=()):
        be = sfmba.Backend(0)
        made.append(be)
        be.set_precision(bits)
        for name, value in options.items():
            be.debug_option(name, value)
        be.set_fixed_cameras(fixed)
        return be
    yield open_
    for be in made:
        be.close()


def _forms(be, want, tag):
    for name, value in want.items():
        assert be.form(name) == value, (tag, name, be.form(name))


def _solve(be, x0, max_nfev=1, **fields):
    opt = be.default_options()
    opt.max_nfev = max_nfev
    for k, v in fields.items():
        setattr(opt, k, v)
    x, res, _, _ = be.solve(x0, opt)
    return x, res, opt


def _state(be):
    """Everything the solve's form keeps (include/sfmba.h: sfmba_get_iteration_state); the refusals have a test of their own."""
    skip = []
    if be.form("dense_solve"):
        skip += ["Minv", "pcg_r"]
    elif not be.form("rhsrec"):
        skip += ["e"]
    if (be.form("pcg_local") or be.form("pcg_local2")) and "pcg_r" not in skip:
        skip += ["pcg_r"]
    try:
        return be.iteration_state(skip=skip)
    except ValueError as err:                             # k_backsub's prologue did the last update (a replayed record)
        assert "pcg_x" in str(err), err
        return be.iteration_state(skip=skip + ["pcg_x"])


def _held(tag, layer, out):
    worst = max(out.values())
    print(f"iteration: {tag} {layer} worst error / bound {worst:.3g}  (" + ", ".join(f"{k} {v:.2g}" for k, v in out.items()) + ")")
    bad = {k: v for k, v in out.items() if not v <= 1.0}
    assert not bad, (tag, layer, bad)


def _layers(tag, be, st, x, opt, C, first=True, prev=0.0, si_old=None, held=(), precond=True):
    """scale, prep and step from the fetched state at the returned x; the blocks are fetched last (normal_blocks computes
    on the handle) -> the blocks."""
    sc = st["scalars"]
    U, V, gc, gp = be.normal_blocks(x)
    _held(tag, "scale", ir.check_scale(st, U, V, gc, gp, x, C, si_old=si_old, held=held))
    _held(tag, "sums", ir.check_scale_sums(sc, st, x, C))
    _held(tag, "prep", ir.check_prep(sc, st, V, gp, C, opt.reg_min, opt.pcg_tol, max(opt.pcg_tol, opt.pcg_tol_max), prev=prev, first=first,
                                     U=None if precond else U))
    _held(tag, "step", ir.check_step(sc))
    _held(tag, "x_new", ir.check_x_new(st["x_new"], x, st["sg"], st["p"], sc[ir.STEP], sc[ir.STEP + 1]))
    return U, V, gc, gp


_LIN = {}


def _lin(problem, orc):
    if problem.startswith(("hand_built", "schur_", "dense_")):
        return eb.linearisation(problem, orc)
    if problem not in _LIN:
        args, x0 = ir.case_problem(problem, orc)
        _LIN[problem] = eb.Linearisation(*args, x0)
    return _LIN[problem]


def _iteration0(tag, be, problem, case, orc, want, held=(), precond=True, dense=False, record=False, second_set=False):
    """The shared body: one outer iteration at x0 on `be`, every layer.  record: a solve with max_nfev = 2 first, so that
    the solve under test replays its record of PCG counts (the speculative launches, FinalUpdate)."""
    args, x0 = ir.case_problem(problem, orc)
    C, P = args[0], args[1]
    be.set_problem(*args)
    _forms(be, want, tag)
    if record:
        _solve(be, x0, max_nfev=2)
        assert be.pcg_history()[0] == ir.load_bounds()["cases"][case]["iters"], tag
    x, res, opt = _solve(be, x0)
    assert np.array_equal(x, x0) and res.nfev == 1, tag
    st = _state(be)
    if record:
        print(f"iteration: {tag} replayed record, pcg_x {'kept' if 'pcg_x' in st else 'refused (FinalUpdate)'}")
    _layers(tag, be, st, x, opt, C, held=held, precond=precond)
    _held(tag, "pcg", ir.check_pcg(case, _lin(problem, orc), st, st["ctrl"], st["scalars"], C, P, held=held, dense=dense, pcg_tol=opt.pcg_tol))
    if second_set:                                       # the speculative k_update_scale: the trial point's set
        U, V, gc, gp = be.normal_blocks(st["x_new"])
        _held(tag, "scale2", ir.check_scale(st, U, V, gc, gp, st["x_new"], C, si_old=st["si"], prefix=("si2", "g2", "sg2")))
    return st


# ---- the hand-built problem in every PCG form -------------------------------------------------------------------------------
HAND_CASES = {      # name -> (debug options, forms, replay a record)
    "default": ({}, dict(LOCAL, skip_last=2), False),
    "pcg_local0": ({"pcg_local": 0}, dict(LOCAL, pcg_local=0, skip_last=1), False),                  # the whole-update prologue
    "pcg_fused0": ({"pcg_fused": 0}, dict(LOCAL, pcg_fused=0, pcg_local=0, pcg_local2=0, skip_last=0), False),   # k_pcg_init + k_pcg_update
    "pcg_split1": ({"pcg_split": 1}, dict(LOCAL, pcg_split=1), False),                                # k_pcg_tail
    "cam_chunk64": ({"cam_chunk": 64}, dict(LOCAL, pcg_split=1, cam_multi=1), False),               # ... behind k_cam_combine
    "cam_chunk64_general": ({"cam_chunk": 64, "pcg_split": 0}, dict(LOCAL, pcg_local=0, pcg_split=0, cam_multi=1), False),
    "record": ({}, dict(LOCAL, skip_last=2), True),                                                   # FinalUpdate of k_backsub
    "record_skip_last0": ({"pcg_skip_last": 0}, dict(LOCAL, skip_last=0), True),                     # every launch enqueued
    "record_skip_last1": ({"pcg_skip_last": 2}, dict(LOCAL, skip_last=1), True),                     # only pass B left out
}


@pytest.mark.parametrize("name", list(HAND_CASES))
def test_hand_built_iteration(opened, orc, name):
    options, forms, record = HAND_CASES[name]
    be = opened(dict(options, dense=0))
    st = _iteration0(name, be, "hand_built", "hand_built", orc, forms, record=record, second_set=name == "default")
    if name in ("pcg_local0", "pcg_fused0", "cam_chunk64_general"):
        assert "pcg_r" in st, name                         # (the residual identity was part of the pcg layer)
    if name == "record":
        assert "pcg_x" not in st, name


PRECOND0_CASES = {  # name -> (debug options, bits, forms)
    "sweep_rc": ({}, 64, dict(sweep_rc=1, round_blocks=0)),                          # k_cam_schur<1,0> behind a recomputing pass A
    "stored": ({"sweep_rc": 0}, 64, dict(sweep_rc=0, sweep_rc_g=0, round_blocks=0)),
    "sweep_rc_whole_update": ({"pcg_local": 0}, 64, dict(sweep_rc=1, pcg_local=0)),   # ... with r kept: the residual identity
    "stored_whole_update": ({"sweep_rc": 0, "pcg_local": 0}, 64, dict(sweep_rc=0, pcg_local=0)),
}


@pytest.mark.parametrize("name", list(PRECOND0_CASES))
def test_block_jacobi_preconditioner_iteration(opened, orc, name):
    """precond = 0: k_prep inverts U + Dc itself (cam_prep_one) and the rhs pass is k_cam_schur<1,0>, pinned by the
    residual identity where the form keeps r."""
    options, bits, forms = PRECOND0_CASES[name]
    be = opened(dict(options, dense=0, precond=0), bits)
    st = _iteration0("precond0_" + name, be, "hand_built", "hand_built_precond0", orc, dict(forms, precond=0, dense_solve=0, pcg_fused=1),
                     precond=False)
    assert ("pcg_r" in st) == name.endswith("whole_update"), name


def test_block_jacobi_preconditioner_fp32_storage(opened, orc):
    """32-bit storage on the stored Jacobian (round_blocks, k_cam_schur<1,1>): the scale, prep and step layers from the
    fetched blocks -- the arithmetic of all three is fp64 whatever the storage -- and the right-hand side of the residual
    identity: with the stored fp32 blocks that residual_jacobian fetches as the operand of both passes (the operator of
    test_product_on_the_stored_fp32_jacobian) and the fetched g_c, g_p, Vinv, r + S x - b = 0 holds only if the rhs pass
    rounded its recomputed blocks as they are stored.  The whole-update form keeps r."""
    args, x0 = ir.case_problem("hand_built", orc)
    C, P = args[0], args[1]
    be = opened({"dense": 0, "precond": 0, "sweep_rc": 0, "pcg_local": 0}, 32)
    be.set_problem(*args)
    _forms(be, dict(precond=0, round_blocks=1, mixed=0, dense_solve=0, pcg_local=0, pcg_fused=1), "fp32")
    x, res, opt = _solve(be, x0)
    st = _state(be)
    U, V, gc, gp = _layers("precond0_stored_fp32", be, st, x, opt, C, precond=False)
    r32, Jc32, Jp32 = be.residual_jacobian(x)
    dp = (st["scalars"][ir.REG] * st["si"][6 * C:]) * st["si"][6 * C:]
    sys_ld = ir.SchurSystem(r32.reshape(-1, 2).astype(ir.LD), Jc32.astype(ir.LD), Jp32.astype(ir.LD), args[2], args[3], C, P, st["Dc"], dp,
                            fetched={"gc": gc, "gp": gp, "Vinv": st["Vinv"]})
    assert np.array_equal(st["pcg_x"], st["p"][:6 * C].reshape(C, 6))
    _held("precond0_stored_fp32", "rhs", ir.check_identity("hand_built_precond0", sys_ld, st))


@pytest.mark.parametrize("name,options,forms", [
    ("schur_1024", {}, dict(LOCAL, skip_last=2)),                                                    # last count of the fused launch
    ("schur_1025", {}, dict(LOCAL, pcg_fused=0, pcg_local=0, pcg_local2=0, skip_last=0, sweep_rc=1)),   # k_pcg_init + k_pcg_update
    ("schur_1025_local2", {"sweep_rc": 2}, dict(LOCAL, pcg_fused=0, pcg_local=0, pcg_local2=1, skip_last=0, sweep_rc_g=1)),   # k_pcg_update_local
])
def test_fused_launch_boundary_iteration(opened, orc, name, options, forms):
    be = opened(dict(options, dense=0))
    _iteration0(name, be, name[:10], name[:10], orc, forms)


def test_dense_path_iteration(opened, orc):
    """21 cameras: k_dense_pcg.  Its preconditioner lives in LDS: the reference inverts the diagonal blocks of its own S."""
    be = opened({})
    st = _iteration0("dense_21", be, "dense_%d" % eb.DENSE_CAMERAS, "dense_21", orc, dict(dense=1, dense_solve=1, one_rank=1), dense=True)
    assert "e" in st and "Minv" not in st


def test_held_cameras_iteration(opened, orc):
    """Cameras 0 and 9 held: scale 1 exactly, no gradient, no step, x_new == x to the bit."""
    held = (0, 9)
    be = opened({"dense": 0}, fixed=held)
    st = _iteration0("held", be, "held", "held", orc, LOCAL, held=held)
    for c in held:
        e = slice(6 * c, 6 * c + 6)
        assert np.all(st["si"][e] == 1.0) and not st["g"][e].any() and not st["sg"][e].any() and not st["p"][e].any(), c
        assert np.array_equal(st["x_new"][e], ir.case_problem("held", orc)[1][e]), c
        assert np.all(st["Dc"][c] == st["scalars"][ir.REG]), c


def test_non_speculative_launches_give_the_same_bits(opened, orc):
    """spec_scale = 0, start_handoff = 0, cost_rider = 0: k_update_scale on the accepted set, a blocking start, k_finish
    posting the cost -- every fetched array as the default form leaves it (the second set is not written there)."""
    args, x0 = ir.case_problem("hand_built", orc)
    states = []
    for options, forms in (({}, dict(quick_start=1, spec_scale=1, cost_rider=1)),
                           ({"spec_scale": 0, "start_handoff": 0, "cost_rider": 0}, dict(quick_start=0, spec_scale=0, cost_rider=0))):
        be = opened(dict(options, dense=0))
        be.set_problem(*args)
        _forms(be, forms, "non_speculative")
        _solve(be, x0)
        states.append(_state(be))
    a, b = states
    assert a["ctrl"] == b["ctrl"]
    differ = [k for k in a if k not in ("ctrl", "si2", "g2", "sg2") and not np.array_equal(a[k], b[k])]
    assert not differ, differ


# ---- beyond iteration 0 -------------------------------------------------------------------------------------------------------
def test_running_maximum_and_adaptive_eta(opened, orc):
    """max_nfev = 2: the first step is accepted and the solve leaves iteration 1.  Its scale is max(sqrt(diag), scale of
    iteration 0), with entries the maximum holds; eta comes from the drop of |g_h|^2 and lies strictly between its limits;
    the set the speculative launch filled at iteration 0 is the set iteration 1 runs on."""
    args, x0 = ir.case_problem("running_max", orc)
    C = args[0]
    be = opened({"dense": 0})
    be.set_problem(*args)
    _forms(be, LOCAL, "running_max")
    _solve(be, x0, max_nfev=1)
    st0 = _state(be)
    x1, res, opt = _solve(be, x0, max_nfev=2)
    assert res.nfev == 2 and res.njev == 2
    st1 = _state(be)
    assert np.array_equal(x1, st0["x_new"])
    for k in ("si", "g", "sg"):
        assert np.array_equal(st1[k], st0[k + "2"]), k
    U, V, gc, gp = _layers("running_max", be, st1, x1, opt, C, first=False, prev=st0["scalars"][ir.GH_PREV], si_old=st0["si"])
    d = np.concatenate([U[:, ir.DIAG_U].ravel(), V[:, ir.DIAG_V].ravel()])
    kept = int((st0["si"] > np.sqrt(d) * (1 + 4 * ir.EPS)).sum())
    eta = st1["scalars"][ir.ETA]
    print(f"iteration: running_max {kept} of {len(d)} scale entries held by the maximum, eta {eta:.6g}, PCG iterations {st1['ctrl']['iters']}")
    assert kept > 0
    assert opt.pcg_tol < eta < opt.pcg_tol_max
    assert st1["ctrl"]["tol2"] == eta * eta


def test_far_start_third_evaluation(opened, orc):
    """max_nfev = 3 on the far start: both steps are accepted there, so the solve leaves iteration 2 with the forcing term
    at its upper limit; scale, prep and step of that iteration from the state of iteration 1."""
    args, x0 = ir.case_problem("far_start", orc)
    C = args[0]
    be = opened({"dense": 0})
    be.set_problem(*args)
    _solve(be, x0, max_nfev=2)
    st1 = _state(be)
    x2, res, opt = _solve(be, x0, max_nfev=3)
    st2 = _state(be)
    assert (res.nfev, res.njev) == (3, 3) and np.array_equal(x2, st1["x_new"])
    _layers("far_start", be, st2, x2, opt, C, first=False, prev=st1["scalars"][ir.GH_PREV], si_old=st1["si"])
    assert st2["scalars"][ir.ETA] == opt.pcg_tol_max


def test_host_retry_after_a_rejected_step(opened, orc):
    """A start whose device-decided first step is rejected: the host re-solves the 2-D model at a quarter of |step_h| and
    k_step_table applies its (c1, c2).  A trial point does not survive a max_nfev break (the next iteration's trial
    overwrites it), so the retry is made the solve's last evaluation: with ftol = 1e30 the first accepted step ends it,
    and the returned x is x0 + c1 sg + c2 p of the state a max_nfev = 1 solve leaves."""
    import sfmba
    pb = sfmba.make_problem(6, 80, 500, seed=8, x0_noise=0.2)
    C = pb.args[0]
    be = opened({"dense": 0})
    be.set_problem(*pb.args)
    _solve(be, pb.x0, max_nfev=1)
    st0 = _state(be)
    sc = st0["scalars"]
    x, res, _ = _solve(be, pb.x0, max_nfev=0, ftol=1e30)
    st = _state(be)
    assert (res.nfev, res.njev, res.status, res.iterations) == (3, 2, 2, 1), (res.nfev, res.njev, res.status, res.iterations)
    assert np.array_equal(st["p"], st0["p"]) and np.array_equal(st["sg2"], st0["sg"]) and np.array_equal(st["x_new"], pb.x0)
    # (the final sums of the accepted point's k_update_scale rewrote slots 8..12 and 16..24: the model is rebuilt from `sc`)
    assert np.array_equal(st["scalars"][1:8], sc[1:8]) and np.array_equal(st["scalars"][25:32], sc[25:32])
    G, a, b = ir.model_inputs(sc)
    ref, bnd = ir.step_bound(G, a, b, 0.25 * sc[ir.STEP + 3])
    assert not np.array_equal(ref[:2].astype(np.float64), sc[ir.STEP:ir.STEP + 2])
    xl, sgl, pl = pb.x0.astype(ir.LD), st0["sg"].astype(ir.LD), st0["p"].astype(ir.LD)
    want = xl + ref[0] * sgl + ref[1] * pl
    bound = 3 * ir.EPS * (np.abs(xl) + np.abs(ref[0] * sgl) + np.abs(ref[1] * pl)) + bnd[0] * np.abs(sgl) + bnd[1] * np.abs(pl)
    _held("host_retry", "x_new", {"x_new": eb.ratio(x, want, bound)})


# ---- two points per thread ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [65536, 65537])
def test_scale_two_points_per_thread(opened, orc, P):
    """From 65536 points on k_update_scale takes two points per thread and trip (kScalePts = 2); 65537 leaves the last
    trip ragged.  8 cameras, two observations a point; scale, prep and step (references of O(n) work)."""
    import sfmba
    C = 8
    pi = np.repeat(np.arange(P), 2)
    ci = np.stack([np.arange(P) % C, (np.arange(P) + 3) % C], axis=1).ravel()
    pb = eb._problem(C, P, ci, pi, sfmba.make_problem(C, P, 2 * P, seed=3), orc, 5, noise=2.0)
    assert "scale_pts = P >= 65536 ? 2 : 1;" in open(os.path.join(ROOT, "sfm-python_amd", "csrc", "sfmba.hip")).read()
    be = opened({"dense": 0})
    be.set_problem(*pb.args)
    _forms(be, dict(one_rank=1, dense_solve=0, quick_start=1, spec_scale=1), P)
    x, res, opt = _solve(be, pb.x0)
    _layers(f"scale_pts2_{P}", be, _state(be), x, opt, C)


# ---- the sharded forms in a world of one ------------------------------------------------------------------------------------------
def test_sharded_world_of_one_iteration(orc):
    """k_finish riders, k_tr_step on 64 threads, the exchanged scalars: scale, prep, step, and dc within the PCG bound of
    the reference (the bound the one-rank case is held to)."""
    from test_gpu_fullsize import sharded_world_of_one, solve_sharded
    pb = eb.hand_built(orc)
    C, P = pb.args[0], pb.args[1]
    with sharded_world_of_one(pb, debug=(("dense", 0),)) as handle:
        be = handle[0]
        _forms(be, dict(one_rank=0, quick_start=0, spec_scale=0, dense_solve=0), "world_of_one")
        (x, res, opt), _ = solve_sharded(handle, lambda b: _solve(b, pb.x0))
        st = _state(be)
        _layers("world_of_one", be, st, x, opt, C)
        _held("world_of_one", "pcg", ir.check_pcg("hand_built", eb.linearisation("hand_built", orc), st, st["ctrl"], st["scalars"], C, P,
                                                  pcg_tol=opt.pcg_tol))


# ---- the entry itself ----------------------------------------------------------------------------------------------------------------
def test_iteration_state_refuses_what_the_form_does_not_keep(opened, orc):
    args, x0 = ir.case_problem("hand_built", orc)
    be = opened({"dense": 0})
    be.set_problem(*args)
    with pytest.raises(ValueError, match="no completed"):
        be.iteration_state()
    _solve(be, x0)
    for name in ("e", "pcg_r"):                            # the local form: pass A overwrote e, r lags one update behind
        with pytest.raises(ValueError, match=name):
            be.iteration_state(skip=[n for n in ("e", "pcg_r") if n != name])
    assert set(be.iteration_state(skip=("e", "pcg_r"))) == set(be.ITERATION_STATE) - {"e", "pcg_r"}
    args, x0 = ir.case_problem("dense_%d" % eb.DENSE_CAMERAS, orc)
    be = opened({})
    be.set_problem(*args)
    _solve(be, x0)
    for name in ("Minv", "pcg_r"):
        with pytest.raises(ValueError, match=name):
            be.iteration_state(skip=[n for n in ("Minv", "pcg_r") if n != name])


def test_iteration_state_leaves_the_handle_as_it_found_it(opened, orc):
    """A solve after sfmba_get_iteration_state returns the bits of the solve without the call."""
    args, x0 = ir.case_problem("hand_built", orc)
    runs = []
    for call in (False, True):
        be = opened({"dense": 0})
        be.set_problem(*args)
        _solve(be, x0)
        if call:
            _state(be)
        opt = be.default_options()
        opt.max_nfev = 6
        xs, res, fun, grad = be.solve(x0, opt)
        runs.append((xs, fun, grad, res.nfev, res.cost, be.pcg_history()))
    a, b = runs
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3:] == b[3:]
