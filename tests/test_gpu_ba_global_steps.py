"""GPU: dvs_ba_solve_global (csrc/ba.hip) ONE trust-region trial step at a time, through dvs_ba_global_step_probe (test library
only: the function the solver's loop itself calls for a trial step), against tests/gba_step_ref.py — the dense longdouble Step of
tests/ba_step_ref.py with the global solver's active set, and the dense restatement of the linear solve of tests/schur_pcg_ref.py.
A whole run corrects a slightly wrong step and converges anyway; one step does not (tests/test_gpu_ba_steps.py).

What this file reaches that no other does: the shared tail of a trial step (k_lm_backsub, k_lm_candidate, the cost, k_lm_norms) and
k_lm_gmax / k_lm_accept with more than 64 cameras and with an INEXACT camera step; the second trip of every loop that strides the
cameras by 256 (k_gba_update, k_lm_norms, k_lm_gmax: "259 cameras", whose cameras 256..258 are free); a K that is no multiple of 4
(k_gba_precond's idle wavefronts: 259 = 4 x 64 + 3, 9 = 4 x 2 + 1); cameras with exactly 63, 64, 65, 255, 256, 257, 512 and 513
observations (k_gba_cam's chunk of up to 256, k_gba_update's fold over chunks, k_gba_precond's stride of 64: "chunk edges");
landmarks with exactly 1, 4, 5, 16, 17 and 20 observations with their rows looked at ("16 free of 20"); a free camera nobody
observes, which is active here and not in the window solver ("edges 8x150"); and a right-hand side that is exactly zero ("b = 0").
tests/test_gba_step_ref_cpu.py asserts those premises and measures GBA_STEP_MEASURED on the CPU.

Bounds are tests/test_gpu_ba_steps.py's (its docstring derives them; the checks are tests/ba_step_checks.py's), with these in place
of the reduced system, which this solver never forms:
* camera rows: the bits of dvs_ba_pcg_probe's x and its iteration count at the same radius and eta; true residual |S x - b| <=
  2 eta |b| against the dense S and iterations within 2 of the restatement's (tests/test_gpu_ba_global.py's rule); rows of fixed
  cameras exactly zero; step[:6K] the bits of -x * scale.
* the whole step at eta = 1e-10: Step.residual <= 10 x GBA_STEP_MEASURED[case, radius].  At eta = 0.1 the step is far from solving
  the system by design; everything that follows from the camera rows is held as tightly as for an exact step.
* model_change against the reference formula on the device's own step, 1e-11 of its absolute terms, and > 0.  A step the PCG left
  cannot tell that formula from one that assumes S x = b (gba_step_ref.ETA_INEXACT says why); test_a_step_that_is_no_pcg_iterate
  gives the hook camera rows that can.

Largest distances on an MI355X (EXPERIMENTS.md, "Global BA step tests", has the table): the step at eta = 1e-10 0.23 of its bound,
the PCG's true residual 0.46 of 2 eta |b|, Vinv 0.077 of its bound, landmark rows 1.1e-15 and model change 1.8e-16 of their absolute
terms, the candidate quaternion 1.6 ulp of its terms, sn / xn 3.8e-16, the candidate's cost 2.2e-16; the device ran the restatement's
number of PCG iterations in every case."""
import numpy as np
import pytest
import ba_step_ref as bs
import ba_step_checks as ck
import gba_step_ref as gs
import schur_pcg_ref as ref
from ba_step_checks import FTOL, PTOL, GTOL, bits, at

pytestmark = pytest.mark.gpu
MARGIN = 10
ETAS = (gs.ETA_INEXACT, gs.ETA_EXACT)
TRIALS = [(n, r, e) for n, r in gs.ALL for e in ETAS]

_BLOCKS, _STEPS, _DENSE, _PCG = {}, {}, {}, {}      # references, computed once and shared (the dense systems live as long as the module)


def problem(name):
    return ref.system_problem("d") if name == "d" else gs.case(name)


def blocks(name):
    """the problem and its Gauss-Newton blocks (H_pp, H_ll, W, g, cost) at the initial point from a plain handle, once per case"""
    from dvslam_amd import BAProblem
    if name not in _BLOCKS:
        P = problem(name)
        _BLOCKS[name] = (P, BAProblem(P).normal_equations())
    return _BLOCKS[name]


def reference(name, radius, o):
    """the reference step of a case's FIRST probe at `radius`, built once from the device's scale and diagonal; a later probe of the
    same case and radius must bring the same bytes of both"""
    P, B = blocks(name)
    key = (name, radius)
    if key not in _STEPS:
        _STEPS[key] = (gs.step(P, *B[:4], radius, scale=o["scale"], diag=o["diag"]), o["scale"].copy(), o["diag"].copy())
    s, sc, dg = _STEPS[key]
    assert (bits(sc) == bits(o["scale"])).all() and (bits(dg) == bits(o["diag"])).all()
    return s


def dense(name, radius):
    """the dense restatement of the linear solve at the initial point, from the device's blocks"""
    key = (name, radius)
    if key not in _DENSE:
        P, B = blocks(name)
        _DENSE[key] = ref.SchurSystem(P, *B[:4], radius)
    return _DENSE[key]


def probe(g, radius, eta, **kw):
    return g.global_step_probe(radius, eta=eta, ftol=FTOL, ptol=PTOL, **kw)


def check_camera_rows(tag, s, o, dist, S=None, eta=None):
    """the camera rows as the PCG left them and as the candidate applies them; S, eta: the dense system to hold them against"""
    K = s.K
    x = o["x"]
    assert np.isfinite(x).all() and not x.reshape(K, 6)[~s.ca].any(), "rows of fixed cameras are exactly zero"
    assert (bits(o["step"][:6 * K]) == bits(-x * o["scale"][:6 * K])).all()
    if S is None:
        return
    bn = np.linalg.norm(S.b)
    true = np.linalg.norm(S.S @ x - S.b)
    if (id(S), eta) not in _PCG:
        _PCG[(id(S), eta)] = S.pcg(eta)
    _, it_ref, rel_ref, ok_ref = _PCG[(id(S), eta)]
    dist["PCG true residual (of 2 eta |b|)"] = float(true / (2 * eta * bn)) if bn > 0 else 0.0
    print(f"{tag}: device {o['pcg_iterations']} iterations, recurrence {o['pcg_rel_residual']:.3e}, true {true / bn if bn > 0 else 0.0:.3e}; "
          f"restatement {it_ref} iterations, {rel_ref:.3e}")
    assert ok_ref == 1 and o["pcg_rel_residual"] <= eta
    assert true <= 2 * eta * bn
    assert abs(o["pcg_iterations"] - it_ref) <= 2


def check_probe(tag, s, o, B, cost_fn, S=None, eta=None, rho=None):
    """every assertion of the module docstring on one probe `o` against the reference `s` (built from o's scale and diag).  rho:
    the bound on the whole step's residual (None: an inexact step).  Returns the distances, in units of their bounds where they
    have one."""
    dist = {}
    assert o["ok"] == 1 and o["finite"] == 1 and o["pcg_ok"] == 1
    lb = s.landmark_blocks()
    ck.check_vinv(tag, s, o, lb, dist)
    check_camera_rows(tag, s, o, dist, S, eta)
    if rho is not None:
        ck.check_step_residual(tag, s, o, rho, dist)
        dist["step"] /= rho
    else:
        assert not o["step"][~s.act].any() and np.isfinite(o["step"]).all()
    ck.check_landmark_rows(tag, s, o, lb, dist)
    ck.check_model_change(tag, s, o, dist)
    assert o["model_change"] > 0
    ck.check_candidate(tag, s, o, dist)
    ck.check_record(tag, s, o, B, cost_fn, dist)
    ck.report(tag, dist, o)
    return dist


def rho_of(name, radius):
    return MARGIN * gs.GBA_STEP_MEASURED[(name, radius)]


@pytest.mark.parametrize("name,radius,eta", TRIALS, ids=[f"{n} r={r:g} eta={e:g}" for n, r, e in TRIALS])
def test_trial_step(gpu, hooks, name, radius, eta):
    """the first trial step of the loop at `radius` (the prologue, then one step), every output of the hook"""
    from dvslam_amd import BAProblem
    P, B = blocks(name)
    g = BAProblem(P, hooks=True)
    o = probe(g, radius, eta)
    ck.check_scale_and_diag(B, o)
    s = reference(name, radius, o)
    x2, it2, rel2, ok2 = BAProblem(P, hooks=True).pcg_probe(radius, eta)
    assert (bits(x2) == bits(o["x"])).all() and it2 == o["pcg_iterations"] and ok2 == o["pcg_ok"]
    assert bits(rel2) == bits(o["pcg_rel_residual"])
    check_probe(f"{name} r={radius:g} eta={eta:g}", s, o, B, ck.cost_of(P), dense(name, radius), eta,
                rho_of(name, radius) if eta == gs.ETA_EXACT else None)
    K = s.K
    if name == "edges 8x150":
        E = bs.EDGES
        e = E["empty_cam"]
        assert o["step"][6 * K + 3 * E["fixed_only_lm"]:][:3].all(), "a landmark seen only by fixed cameras moves"
        assert s.ca[e] and not o["step"][6 * e:][:6].any(), "an active camera nobody observes: b_c = 0, a zero step"
        assert (bits(o["q"][e]) == bits(P["q"][e])).all() and (bits(o["t"][e]) == bits(P["t"][e])).all()
        wca, wla, _ = bs.active_blocks(P)
        xn_window = float((P["q"][wca] ** 2).sum() + (P["t"][wca] ** 2).sum() + (P["X"][wla] ** 2).sum())
        print(f"{name}: xn {o['xn']!r}, by the window solver's rule {xn_window!r}")
        assert abs(o["xn"] - xn_window) > 1e-6 * o["xn"], "its |x|^2 is in xn all the same (held to 1e-13 above): the window rule is far off"
    if name == "16 free of 20":
        nobs = np.bincount(P["lm_idx"], minlength=s.L)
        assert sorted(set(nobs.tolist())) == [1, 4, 5, 16, 17, 20] and o["step"][6 * K:].all()
    qp, tp, Xp = g.parameters()                                  # the handle's parameters stay the problem's
    assert (bits(qp) == bits(P["q"])).all() and (bits(tp) == bits(P["t"])).all() and (bits(Xp) == bits(P["X"])).all()


@pytest.mark.parametrize("name", gs.STRIDES)
def test_a_step_that_is_no_pcg_iterate(gpu, hooks, name):
    """"The model cost change is computed from the actual step, so it is right for an inexact one" (include/dvslam_hip.h).  A step the
    PCG left satisfies x.(S x - b) = 0, which makes a formula that assumes S x = b right as well; camera rows given to the hook in
    place of the PCG's (gba_step_ref.off_krylov_rows of the device's own eta = 0.1 iterate) do not.  The tail of the trial step runs
    on them: landmark rows, model_change from the step actually taken, candidate, norms, cost, verdict."""
    from dvslam_amd import BAProblem
    P, B = blocks(name)
    g = BAProblem(P, hooks=True)
    a = probe(g, 1e4, gs.ETA_INEXACT)
    xin = gs.off_krylov_rows(a["x"])
    o = probe(g, 1e4, gs.ETA_INEXACT, x_in=xin)
    s = reference(name, 1e4, o)
    assert (bits(o["x"]) == bits(xin)).all() and o["pcg_iterations"] == 0
    check_probe(f"{name} given rows", s, o, B, ck.cost_of(P))
    mc, mmag = s.model_change(o["step"])
    short = gs.exact_solve_model_change(s, o["step"])
    mca, mmaga = s.model_change(a["step"])
    shorta = gs.exact_solve_model_change(s, a["step"])
    print(f"{name}: the PCG's own step: model change and the exact-solve shortcut {float(abs(mca - shorta) / mmaga):.2e} of the absolute terms "
          f"apart; the given rows: {float(abs(mc - short) / mmag):.2e} (bound on model_change 1e-11)")
    assert abs(mca - shorta) <= 1e-11 * mmaga, "the PCG's own iterate cannot tell the two"
    assert abs(mc - short) > 1e3 * 1e-11 * mmag, "premise: these rows can"


@pytest.mark.parametrize("name", gs.TWO_SOLVERS)
def test_both_solvers_on_one_window(gpu, hooks, name):
    """a window both device solvers take, with the same active set in both: the global probe at eta = 1e-10 and the window solver's
    step_probe lie within their own bounds of the SAME reference step, and scale and diag have the same bytes (both come from
    k_lm_scale and k_lm_observations on the same blocks; nothing in them depends on the solver)"""
    from dvslam_amd import BAProblem
    P, B = blocks(name)
    o = probe(BAProblem(P, hooks=True), 1e4, gs.ETA_EXACT)
    w = BAProblem(P, hooks=True).step_probe(1e4, ftol=FTOL, ptol=PTOL)
    assert (bits(o["scale"]) == bits(w["scale"])).all() and (bits(o["diag"]) == bits(w["diag"])).all()
    ck.check_scale_and_diag(B, o)
    s = reference(name, 1e4, o)
    assert (s.ca == bs.active_blocks(P)[0]).all()
    rg, rw = s.residual(o["step"]), s.residual(w["step"])
    print(f"{name}: residual of the global step {rg:.2e} ({rg / rho_of(name, 1e4):.2e} of its bound), of the window solver's {rw:.2e} "
          f"({rw / (MARGIN * bs.STEP_MEASURED[1e4]):.2e} of its bound)")
    assert rg <= rho_of(name, 1e4) and rw <= MARGIN * bs.STEP_MEASURED[1e4]
    assert not o["step"][~s.act].any() and not w["step"][~s.act].any()
    assert (bits(o["x_cost"]) == bits(w["x_cost"])).all() and (bits(o["gmax"]) == bits(w["gmax"])).all()


def _residual_with_diag(s, delta, diag):
    """Step.residual of delta if the LM diagonal were `diag` instead of s.diag"""
    d = s.scaled(delta)[s.idx]
    D = np.asarray(diag, bs.LD)[s.idx] / bs.LD(s.radius)
    gsv = s.gs[s.idx]
    r = np.abs(s.Hs @ d + D * d + gsv)
    return float((r / (np.abs(s.Hs) @ np.abs(d) + D * np.abs(d) + np.abs(gsv))).max())


@pytest.mark.parametrize("name", gs.STRIDES)
def test_rejected_step_reuses_the_diagonal(gpu, hooks, name):
    """tests/test_gpu_ba_steps.py's test of the same name, for the global hook: the same point at half the radius with the diagonal
    KEPT; then, after an accepted step, refresh still off: the diagonal keeps the OLD point's bytes and the step is the reference's
    with that frozen diagonal on the NEW point's blocks"""
    from dvslam_amd import BAProblem
    P, B = blocks(name)
    g = BAProblem(P, hooks=True)
    r, eta = 2e4, gs.ETA_EXACT
    a = probe(g, r, eta)
    b = probe(g, r / 2, eta, refresh=False)
    assert (bits(b["diag"]) == bits(a["diag"])).all() and (bits(b["scale"]) == bits(a["scale"])).all()
    ck.check_scale_and_diag(B, b)
    s = reference(name, r / 2, b)
    rho = rho_of(name, r / 2)
    check_probe(f"{name} r/2, diagonal kept", s, b, B, ck.cost_of(P), dense(name, r / 2), eta, rho)
    c = probe(g, r / 2, eta, commit=True)
    assert c["accept"] == 1 and (bits(c["step"]) == bits(b["step"])).all(), "the same trial again, now committed"
    Pn = at(P, c["q"], c["t"], c["X"])
    Bn = BAProblem(Pn).normal_equations()
    d = probe(g, r / 2, eta, refresh=False)
    assert (bits(d["diag"]) == bits(a["diag"])).all(), "refresh = 0 keeps the stored diagonal"
    fresh = bs.lm_diagonal(Bn[0], Bn[1], a["scale"])
    assert (np.abs(fresh - a["diag"]) > 1e-9 * fresh).any(), "premise: a rebuilt diagonal would differ"
    s3 = gs.step(Pn, *Bn[:4], r / 2, scale=a["scale"], diag=a["diag"])
    check_probe(f"{name} new point, old diagonal", s3, d, Bn, ck.cost_of(P), rho=rho)
    assert _residual_with_diag(s3, d["step"], fresh) > rho, "premise: with a rebuilt diagonal the step would be another"


@pytest.mark.parametrize("name", gs.STRIDES)
def test_committed_step_is_the_next_iteration(gpu, hooks, name):
    """probe with commit on a step the reference accepts: the next probe starts from the candidate with the scaling frozen and the
    diagonal rebuilt from the new blocks, and its step is the reference's at the new point with the old scale"""
    from dvslam_amd import BAProblem
    P, B = blocks(name)
    g = BAProblem(P, hooks=True)
    eta = gs.ETA_EXACT
    a = probe(g, 1e4, eta, commit=True)
    s = reference(name, 1e4, a)
    cq, ct, cX = s.candidate(s.delta)
    ref_rec = dict(ok=1, finite=1, model_change=float(s.model_change(s.delta)[0]), x_cost=B[4], cand_cost=ck.cost_of(P)(cq, ct, cX))
    ref_rec["sn"], ref_rec["xn"] = (float(v) for v in s.norms(cq, ct, cX))
    assert bs.accept_rule(ref_rec, FTOL, PTOL) == 1, "premise: the reference accepts this step"
    assert a["accept"] == 1
    Pn = at(P, a["q"], a["t"], a["X"])
    Bn = BAProblem(Pn).normal_equations()
    b = probe(g, 1e4, eta)
    ck.check_scale_and_diag(Bn, b, scale_from=a["scale"])
    assert (bits(b["diag"]) != bits(a["diag"])).any()
    s2 = gs.step(Pn, *Bn[:4], 1e4, scale=a["scale"], diag=b["diag"])
    check_probe(f"{name} second iteration", s2, b, Bn, ck.cost_of(P), rho=rho_of(name, 1e4))
    qp, tp, Xp = g.parameters()
    assert (bits(qp) == bits(P["q"])).all() and (bits(tp) == bits(P["t"])).all() and (bits(Xp) == bits(P["X"])).all()


@pytest.mark.parametrize("name", gs.STRIDES + ("d",))
def test_replayed_solve_is_bit_identical(gpu, hooks, name):
    """solve_global(max_iterations=10) replayed through the hook with commit reproduces that solve's trace(), pcg_trace() and
    parameters bit for bit: the loop and the hook run the same launches.  "259 cameras" rejects three steps in a row on the way
    (kinds 1 1 1 1 2 2 2 1 1 1), so the kept diagonal and the shrinking radius are part of the replay; (d) is schur_pcg_ref's,
    whose run at the default eta accepts eight steps and ends on the function tolerance (kind 4) in the ninth, so that exit is."""
    import ba_bracket as bb
    from dvslam_amd import BAProblem
    P, _ = blocks(name)
    a = BAProblem(P, hooks=True); b = BAProblem(P, hooks=True)
    sa = a.solve_global(max_iterations=10, function_tolerance=FTOL, gradient_tolerance=GTOL, parameter_tolerance=PTOL)
    rows, q, t, X, probes = ck.replay(lambda radius, refresh, commit: probe(b, radius, 0.1, refresh=refresh, commit=commit), P, 10)
    tr = a.trace()
    its, rels = a.pcg_trace()
    print(f"({name}) {len(tr)} iterations, kinds {tr[:, 1].astype(int).tolist()}, PCG iterations {its.tolist()}")
    assert len(tr) == sa.ba.num_iterations == len(rows) and len(its) == len(probes)
    if name == "259 cameras":
        assert (tr[:, 1] == 2).any() and (tr[:, 1] == 1).any(), "premise: rejected steps"
    if name == "d":
        assert tr[-1, 1] == 4 and len(tr) < 10 and (tr[:-1, 1] == 1).all(), "premise: the function-tolerance exit"
    assert (bits(rows) == bits(tr)).all(), np.nonzero(bits(rows) != bits(tr))
    assert [o["pcg_iterations"] for o in probes] == its.tolist() and sum(its.tolist()) == sa.pcg_iterations
    assert (bits(np.array([o["pcg_rel_residual"] for o in probes])) == bits(rels)).all()
    for x, y in zip((q, t, X), a.parameters()):
        assert (bits(x) == bits(y)).all()
    bb.check_schedule(tr)


def test_zero_right_hand_side(gpu, hooks):
    """"b = 0": no free camera is coupled to an active landmark.  x = 0 IS the solution: zero iterations, a VALID step whose landmark
    rows are the back-substitution of -Vinv g_l, and the solve makes progress (it used to take the breakdown exit before the first
    iteration, call every trial invalid and fail after five of them)"""
    from dvslam_amd import BAProblem
    name = "b = 0"
    P, B = blocks(name)
    g = BAProblem(P, hooks=True)
    o = probe(g, 1e4, 0.1)
    K = int(P["K"])
    assert (o["pcg_ok"], o["pcg_iterations"], o["pcg_rel_residual"]) == (1, 0, 0.0)
    assert not o["x"].any() and not o["step"][:6 * K].any() and o["step"][6 * K:].all()
    ck.check_scale_and_diag(B, o)
    s = reference(name, 1e4, o)
    S = dense(name, 1e4)
    assert not S.b.any()
    check_probe(name, s, o, B, ck.cost_of(P), S, 0.1, rho_of(name, 1e4))
    x2, it2, rel2, ok2 = BAProblem(P, hooks=True).pcg_probe(1e4, 0.1)
    assert (it2, rel2, ok2) == (0, 0.0, 1) and not x2.any()
    h = BAProblem(P)
    sm = h.solve_global()
    tr = h.trace()
    print(f"b = 0: solve_global: termination {sm.ba.termination}, {sm.ba.num_successful_steps} successful steps of {sm.ba.num_iterations}, "
          f"cost {sm.ba.initial_cost!r} -> {sm.ba.final_cost!r}, {sm.pcg_iterations} PCG iterations")
    assert sm.ba.termination != 2 and sm.ba.num_successful_steps >= 1 and sm.ba.final_cost < sm.ba.initial_cost
    assert sm.pcg_iterations == 0 and (tr[:, 1] != 0).all()
    q, t, X = h.parameters()
    assert (bits(q) == bits(P["q"])).all() and (bits(t) == bits(P["t"])).all() and (X != P["X"]).any(axis=1).all()
