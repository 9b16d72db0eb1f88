"""GPU: dvs_ba_solve_device (csrc/ba.hip, the k_lm_* kernels) ONE Levenberg-Marquardt trial step at a time, through
dvs_ba_step_probe (test library only: the functions the solver's loop itself calls to enqueue its launches), against the dense
longdouble reference tests/ba_step_ref.py.  A whole run corrects a slightly wrong step and converges anyway; one step does not.

Both sides start from the same numbers: the Gauss-Newton blocks are those of dvs_ba_normal_equations at the point (held to the
oracle at 1e-12 by tests/test_gpu_ba.py), and the reference takes the device's scale and LM diagonal once they have passed their own
check.  The windows, what each is for and the measured constants are ba_step_ref.CASES / STEP_MEASURED
(tests/test_ba_step_ref_cpu.py asserts the premises and re-measures the constants on the CPU).

Bounds, per probe (eps = 2^-52):
* scale, diag, S, rhs: |got - want| <= 1e-11 x the sum of the absolute values of the terms, element by element — the form and the
  constant tests/test_gpu_ba_global.py::test_operator_preconditioner_and_rhs derives (about 5e4 eps against at most a few thousand
  summed terms).
* Vinv by its residual.  The kernel forms adjugate / determinant in float64 from V rounded to float64 (3 roundings per entry).
  A cofactor c = p1 - p2 is then off by at most 9u (|p1| + |p2|) (u = eps / 2: the inputs' 6u, two products, one difference), the
  determinant's expansion by at most 12u x the sum of its absolute terms, the division adds u.  With G and tau of
  ba_step_ref.inv3_rounding, Vinv_dev - Vinv = dC / det - Vinv (d det / det) + u-terms, and since V Vinv = I
      |V Vinv_dev - I| <= 9u |V| G + 12u tau I + 2u |V| |Vinv|  <=  16 eps (|V| G + tau I).
  Both |V| G and tau are at most about cond(V) (and are of that size when V is close to singular): the residual is held against
  cond(V), whatever the damping; the print-out shows cond(V) beside it.
* the step: Step.residual <= 10 x STEP_MEASURED[radius] — the full-system residual of a plain float64 Schur solve, measured on
  the CPU, times the margin the pose-graph and RANSAC stage tests give a kernel that evaluates the same formulas in another order.
* the landmark rows alone, from the device's own camera rows and its own Vinv: 1e-11 x the absolute terms (k_lm_backsub's sums).
* model_change: against the reference formula on the device's own step, 1e-11 x (|d|.|g_s| + |d|^T |H_s| |d| / 2); against the
  reference step's value, Step.model_change_slack at the step bound on top of that.
* candidate: t + d and X + d are one IEEE addition of float64 numbers the hook returns, so they are compared bit for bit.  The
  quaternion is four sums of four products of (sin(|d|) / |d|) d, cos(|d|) with x: |d| carries 3u (three squares, two additions, a
  square root), which moves sin and cos by at most 3u |d|; sin, cos of the device library 2u each; the quotient, the product with d,
  the product with x and three additions one u each: 14u + 3u |d| of the sum of the absolute products, plus u for the reference's
  own rounding to float64: within (8 + 2 |d|) eps of ba_step_ref.quat_plus_magnitude, i.e. 8 ulp for the steps of these windows.
  Inactive blocks keep their bytes.
* sn, xn: numpy (longdouble) on the device's candidate, 1e-13 relative.  cand_cost: a fresh handle's evaluate() at the candidate,
  1e-12 relative (tests/test_gpu_ba_global.py: cost-only against full evaluation).  x_cost: the bits of the blocks' cost.  gmax: the
  reference's, within the quaternion bound above (a maximum is 1-Lipschitz).  accept: the loop's rule on the record's own numbers."""
import numpy as np
import pytest
import ba_step_ref as bs
import ba_step_checks as ck
from ba_step_checks import FTOL, PTOL, GTOL, check_scale_and_diag

pytestmark = pytest.mark.gpu
EPS = bs.EPS
LD = bs.LD
MARGIN = 10
ALL = [(n, r) for n, (_, _, radii) in bs.CASES.items() for r in radii]
_bits, _at, _cost_of = ck.bits, ck.at, ck.cost_of


def _handle(P, name, hooks=True):
    from dvslam_amd import BAProblem
    g = BAProblem(P, hooks=hooks)
    if bs.CASES[name][1] != 16:
        g.set_device_window(bs.CASES[name][1])
    return g


_BLOCKS = {}


def blocks(name):
    """the window and its Gauss-Newton blocks (H_pp, H_ll, W, g, cost) at the initial point from a plain handle, once per case"""
    from dvslam_amd import BAProblem
    if name not in _BLOCKS:
        P = bs.case(name)
        _BLOCKS[name] = (P, BAProblem(P).normal_equations())
    return _BLOCKS[name]


_STEPS = {}


def reference(name, radius, o):
    """the reference step of a case's FIRST probe at `radius`, built once from the device's scale and diagonal; a later probe of the
    same case and radius must bring the same bytes of both"""
    P, B = blocks(name)
    key = (name, radius)
    if key not in _STEPS:
        _STEPS[key] = (bs.Step(P, *B[:4], P["q"], P["t"], P["X"], radius, scale=o["scale"], diag=o["diag"]), o["scale"].copy(), o["diag"].copy())
    s, sc, dg = _STEPS[key]
    assert (_bits(sc) == _bits(o["scale"])).all() and (_bits(dg) == _bits(o["diag"])).all()
    return s


def check_probe(tag, s, o, B, cost_of):
    """every assertion of the module docstring on one probe `o` against the reference `s` (built from o's scale and diag);
    cost_of(q, t, X): a fresh handle's evaluate() cost.  The pieces the global solver's step tests share are ba_step_checks'.
    Returns the distances, in units of their bounds where they have one."""
    dist = {}
    assert o["ok"] == 1 and o["finite"] == 1
    # ---- reduced system
    red = s.reduced()
    n = 6 * len(s.slots)
    assert o["S"].shape == (n, n)
    low = np.arange(n)[None, :] < 6 * (np.arange(n)[:, None] // 6) + 6
    assert not o["S"][~low].any()
    eS = np.abs(o["S"] - red["S"])[low] / red["Smag"][low]
    er = np.abs(o["rhs"] - red["rhs"]) / red["rhsmag"]
    dist["S"], dist["rhs"] = float(eS.max()), float(er.max())
    assert dist["S"] <= 1e-11, f"{tag}: S off by {dist['S']:.2e} of the un-cancelled magnitude"
    assert dist["rhs"] <= 1e-11, f"{tag}: rhs off by {dist['rhs']:.2e} of the un-cancelled magnitude"
    ck.check_vinv(tag, s, o, red, dist)
    # ---- the step
    rho = MARGIN * bs.STEP_MEASURED[s.radius]
    ck.check_step_residual(tag, s, o, rho, dist)
    ck.check_landmark_rows(tag, s, o, red, dist)
    # ---- model cost change
    mmag = ck.check_model_change(tag, s, o, dist)
    mc_ref, _ = s.model_change(s.delta)
    assert abs(o["model_change"] - mc_ref) <= s.model_change_slack(o["step"], rho) + 1e-11 * mmag
    ck.check_candidate(tag, s, o, dist)
    ck.check_record(tag, s, o, B, cost_of, dist)
    ck.report(tag, dist, o)
    return dist


@pytest.mark.parametrize("name,radius", ALL, ids=[f"{n} r={r:g}" for n, r in ALL])
def test_trial_step(gpu, hooks, name, radius):
    """the first trial step of the loop at `radius` (the prologue, then one step), every output of the hook"""
    P, B = blocks(name)
    g = _handle(P, name)
    o = g.step_probe(radius, ftol=FTOL, ptol=PTOL)
    check_scale_and_diag(B, o)
    s = reference(name, radius, o)
    check_probe(f"{name} r={radius:g}", s, o, B, _cost_of(P))
    if name == "edges 8x150":
        E = bs.EDGES
        K = s.K
        lone = o["step"][6 * K + 3 * E["fixed_only_lm"]:][:3]
        assert lone.all(), "a landmark seen only by fixed cameras moves"
        assert not o["step"][6 * E["empty_cam"]:][:6].any(), "a free camera without observations has no slot"
        assert (_bits(o["q"][E["empty_cam"]]) == _bits(P["q"][E["empty_cam"]])).all()
    qp, tp, Xp = g.parameters()                                  # the handle's parameters stay the problem's
    assert (_bits(qp) == _bits(P["q"])).all() and (_bits(tp) == _bits(P["t"])).all() and (_bits(Xp) == _bits(P["X"])).all()


@pytest.mark.parametrize("name", bs.REPLAY)
def test_rejected_step_reuses_the_diagonal(gpu, hooks, name):
    """the loop after a rejected step: the same point at half the radius with the diagonal KEPT.  Then the same after an accepted
    step with refresh still off — not something the loop does, but the only way to see that `refresh = 0` reads the stored diagonal
    (at an unchanged point a rebuilt diagonal has the same bytes): the diagonal keeps the OLD point's bytes and the step is the
    reference's with that frozen diagonal on the NEW point's blocks."""
    from dvslam_amd import BAProblem
    P, B = blocks(name)
    g = _handle(P, name)
    r = 2e4
    a = g.step_probe(r, ftol=FTOL, ptol=PTOL)
    b = g.step_probe(r / 2, refresh=False, ftol=FTOL, ptol=PTOL)
    assert (_bits(b["diag"]) == _bits(a["diag"])).all() and (_bits(b["scale"]) == _bits(a["scale"])).all()
    check_scale_and_diag(B, b)
    s = reference(name, r / 2, b)
    check_probe(f"{name} r/2, diagonal kept", s, b, B, _cost_of(P))
    # an accepted step, then refresh = 0 at the new point
    c = g.step_probe(r / 2, commit=True, ftol=FTOL, ptol=PTOL)
    assert c["accept"] == 1 and (_bits(c["step"]) == _bits(b["step"])).all(), "the same trial again, now committed"
    Pn = _at(P, c["q"], c["t"], c["X"])
    Bn = BAProblem(Pn).normal_equations()
    d = g.step_probe(r / 2, refresh=False, ftol=FTOL, ptol=PTOL)
    assert (_bits(d["diag"]) == _bits(a["diag"])).all(), "refresh = 0 keeps the stored diagonal"
    fresh = bs.lm_diagonal(Bn[0], Bn[1], a["scale"])
    assert (np.abs(fresh - a["diag"]) > 1e-9 * fresh).any(), "premise: a rebuilt diagonal would differ"
    s3 = bs.Step(Pn, *Bn[:4], Pn["q"], Pn["t"], Pn["X"], r / 2, scale=a["scale"], diag=a["diag"])
    check_probe(f"{name} new point, old diagonal", s3, d, Bn, _cost_of(P))
    s4 = bs.Step(Pn, *Bn[:4], Pn["q"], Pn["t"], Pn["X"], r / 2, scale=a["scale"])
    assert s4.residual(d["step"]) > MARGIN * bs.STEP_MEASURED[r / 2], "premise: with a rebuilt diagonal the step would be another"


@pytest.mark.parametrize("name", bs.REPLAY)
def test_committed_step_is_the_next_iteration(gpu, hooks, name):
    """probe with commit on a step the reference accepts: the next probe starts from the candidate with the scaling frozen and the
    diagonal rebuilt from the new blocks, and its step is the reference's at the new point with the old scale"""
    from dvslam_amd import BAProblem
    P, B = blocks(name)
    g = _handle(P, name)
    a = g.step_probe(1e4, commit=True, ftol=FTOL, ptol=PTOL)
    s = reference(name, 1e4, a)
    cq, ct, cX = s.candidate(s.delta)
    ref_rec = dict(ok=1, finite=1, model_change=float(s.model_change(s.delta)[0]), x_cost=B[4], cand_cost=_cost_of(P)(cq, ct, cX))
    ref_rec["sn"], ref_rec["xn"] = (float(v) for v in s.norms(cq, ct, cX))
    assert bs.accept_rule(ref_rec, FTOL, PTOL) == 1, "premise: the reference accepts this step"
    assert a["accept"] == 1
    Pn = _at(P, a["q"], a["t"], a["X"])
    Bn = BAProblem(Pn).normal_equations()
    r2 = 1e4                                                      # (the loop would go on at up to 3e4; any radius shows the state)
    b = g.step_probe(r2, ftol=FTOL, ptol=PTOL)
    check_scale_and_diag(Bn, b, scale_from=a["scale"])
    assert (_bits(b["diag"]) != _bits(a["diag"])).any()
    s2 = bs.Step(Pn, *Bn[:4], Pn["q"], Pn["t"], Pn["X"], r2, scale=a["scale"], diag=b["diag"])
    check_probe(f"{name} second iteration", s2, b, Bn, _cost_of(P))


def _replay(g, P, iters):
    """dvs_ba_solve_device's loop around the hook (ba_step_checks.replay): -> (trace rows, q, t, X)"""
    return ck.replay(lambda radius, refresh, commit: g.step_probe(radius, refresh=refresh, commit=commit, ftol=FTOL, ptol=PTOL), P, iters)[:4]


@pytest.mark.parametrize("name", bs.REPLAY + ("hard 5x200",))
def test_replayed_solve_is_bit_identical(gpu, hooks, name):
    """solve_device(10) replayed through the hook reproduces that solve's trace() and parameters bit for bit ("hard 5x200":
    ba_bracket.HARD[0] for 40 iterations, whose run rejects steps, so the kept diagonal and the shrinking radius are part of the
    replay)"""
    import ba_bracket as bb
    from dvslam_amd import BAProblem, synth
    if name.startswith("hard"):
        P = synth.make_ba_problem(**bb.HARD[0]); a = BAProblem(P, hooks=True); b = BAProblem(P, hooks=True)
    else:
        P, _ = blocks(name); a = _handle(P, name); b = _handle(P, name)
    iters = 40 if name.startswith("hard") else 10
    sa = a.solve_device(iters, FTOL, GTOL, PTOL)
    rows, q, t, X = _replay(b, P, iters)
    tr = a.trace()
    print(f"{name}: {len(tr)} iterations, kinds {tr[:, 1].astype(int).tolist()}")
    assert len(tr) == sa.num_iterations == len(rows)
    if name.startswith("hard"):
        assert (tr[:, 1] == 2).any() and (tr[:, 1] == 1).any()
    assert (_bits(rows) == _bits(tr)).all(), np.nonzero(_bits(rows) != _bits(tr))
    for x, y in zip((q, t, X), a.parameters()):
        assert (_bits(x) == _bits(y)).all()
    bb.check_schedule(tr)


@pytest.mark.parametrize("solver", ["solve", "solve_device"])
@pytest.mark.parametrize("name", ["live 5x200", "edges 8x150"])
def test_first_iteration_without_the_hook(gpu, name, solver):
    """solve(1) (the host-Schur path) and solve_device(1) on the product library: trace row 0 and the parameters afterwards against
    the reference step at radius 1e4.  The solver's own step is not visible here; it is a float64 Schur solve, within
    rho = 10 x STEP_MEASURED[1e4] of the exact step in the residual distance, i.e. within e = |A^-1| rho magnitude of it row by row.
    From that: the model change within model_change_slack (+ 1e-11 of its absolute terms), the candidate's cost within
    2 |g(candidate)| . e (+ 1e-12 relative), an accepted point within 2 e (quaternions: 2 |q| |e_rot|_1) of the reference's
    candidate; a rejected step leaves the initial bytes."""
    from dvslam_amd import BAProblem
    P, B = blocks(name)
    s = bs.Step(P, *B[:4], P["q"], P["t"], P["X"], 1e4)
    g = BAProblem(P)
    getattr(g, solver)(1, FTOL, GTOL, PTOL)
    row = g.trace()[0]
    assert len(g.trace()) == 1 and row[0] == 1e4 and int(row[1]) in (1, 2)
    rho = MARGIN * bs.STEP_MEASURED[1e4]
    mc, mmag = s.model_change(s.delta)
    slack = s.model_change_slack(s.delta, rho) + 1e-11 * float(mmag)
    cq, ct, cX = s.candidate(s.delta)
    cand_cost, _, _, _, gc = BAProblem(_at(P, cq, ct, cX)).evaluate()
    e = np.zeros(s.N)
    e[s.idx] = (np.abs(s.Ainv) @ (rho * s.magnitude(s.delta)).astype(np.float64)) * s.scale[s.idx].astype(np.float64)
    dcost = 2 * float(np.abs(gc) @ e) + 1e-12 * cand_cost
    print(f"{name} {solver}: model change {row[3]!r} / {float(mc)!r} (slack {slack:.2e}); candidate cost {row[5]!r} / {cand_cost!r} (slack {dcost:.2e})")
    assert abs(row[3] - float(mc)) <= slack
    assert abs(row[5] - cand_cost) <= dcost
    rel = (B[4] - cand_cost) / float(mc)
    assert (int(row[1]) == 1) == (rel > 1e-3) and abs(row[4] - rel) <= (dcost + abs(rel) * slack) / float(mc) + 1e-12 * abs(rel)
    q, t, X = g.parameters()
    if int(row[1]) == 1:
        K = s.K
        ec = e[:6 * K].reshape(K, 6)
        assert (np.abs(t - ct) <= 2 * ec[:, 3:] + 4 * EPS * np.abs(ct)).all()
        assert (np.abs(X - cX) <= 2 * e[6 * K:].reshape(s.L, 3) + 4 * EPS * np.abs(cX)).all()
        assert (np.abs(q - cq) <= (2 * ec[:, :3].sum(1) + 16 * EPS)[:, None] * np.abs(P["q"]).sum(1)[:, None]).all()
        assert (_bits(q[~s.ca]) == _bits(P["q"][~s.ca])).all() and (_bits(X[~s.la]) == _bits(P["X"][~s.la])).all()
        assert (q[s.ca] != P["q"][s.ca]).any(axis=1).all() and (X[s.la] != P["X"][s.la]).any(axis=1).all()
    else:
        assert (_bits(q) == _bits(P["q"])).all() and (_bits(t) == _bits(P["t"])).all() and (_bits(X) == _bits(P["X"])).all()
