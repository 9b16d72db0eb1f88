"""The step-level statements of tests/pose_graph_ref.py without a GPU: the graphs that make the pose-graph solver reject, fail, stop by the
parameter tolerance and make a second trip through its single-workgroup loops; the premises that keep every decision of the replayed
steps away from its threshold (so that tests/test_gpu_pose_graph_steps.py can demand equal decisions from the device); trial_step() against
the restatement's own loop; and the constants the GPU step tests hold the device to, re-measured:
  TRIAL_MEASURED     trial_step() in float64 against trial_step() in numpy.longdouble at the same poses and step, in the distance
                     pose_graph_ref.trial_distance states, over every replayed step of every case;
  PCG_STEP_MEASURED  the restatement's float64 PCG against pcg_k() in longdouble on the same float64 system, stopped at the same iteration,
                     |x - x_ld| / |x_ld|, per graph."""
import warnings
import numpy as np
import pytest

import pose_graph_ref as pr


def _kinds(trace):
    return tuple(int(r[1]) for r in trace)


def test_ring24_far_rejects_four_times_in_a_row_and_once_alone():
    s = pr.solve_case("ring24_far")
    kinds = _kinds(s["trace"])
    print("ring24_far kinds", kinds)
    assert kinds[:12] == pr.FAR_KINDS
    assert kinds[4:8] == (2, 2, 2, 2) and kinds[9:12] == (1, 2, 1)
    st = s["steps"]
    # the radius is divided by 2, 4, 8, 16 and the diagonal is kept from the second of the four trials on
    assert [st[k]["radius"] / st[k + 1]["radius"] for k in range(4, 8)] == [2.0, 4.0, 8.0, 16.0]
    assert [st[k]["reuse"] for k in range(4, 9)] == [False, True, True, True, True] and not st[9]["reuse"]
    assert all(st[k]["D"] is st[4]["D"] and st[k]["q"] is st[4]["q"] for k in range(5, 9))
    assert s["termination"] == 0 and kinds[-1] == 4 and s["num_iterations"] == 83 and s["num_successful_steps"] == 71
    assert abs(s["final_cost"] - 19110.21) < 0.01


def test_ring24_far2_rejects_after_the_first_accept_and_meets_the_iteration_limit():
    s = pr.solve_case("ring24_far2")
    kinds = _kinds(s["trace"])
    assert kinds[:6] == pr.FAR2_KINDS
    assert s["termination"] == 1 and s["num_iterations"] == 100


def test_chain515_makes_a_second_trip_and_converges():
    g = pr.graph("chain515")
    assert (g.N, g.E) == (515, 517) and g.N - 512 == 3 and g.E - 512 == 5
    s = pr.solve_case("chain515")
    kinds = _kinds(s["trace"])
    print("chain515 kinds", kinds, "cost", s["final_cost"])
    assert s["termination"] == 0 and kinds == (1,) * 19 + (4,) and abs(s["final_cost"] - 7.0253) < 1e-4
    gf = pr.graph("chain515_fixed")
    assert gf.fixed[513] == 1 and gf.fixed.sum() == 2 and (gf.ei == g.ei).all()


def test_parameter_tolerance_ends_ring24_at_step_five():
    s = pr.solve_case("ring24_ptol")
    assert _kinds(s["trace"]) == (1, 1, 1, 1, 3) and s["termination"] == 0 and s["num_iterations"] == 5
    assert all(st["ptol_margin"] > pr.PREMISE and st["pcg_margin"] > pr.PREMISE and st["rho_margin"] > pr.PREMISE for st in s["steps"])


def test_overflowing_weights_fail_after_five_invalid_steps():
    g = pr.graph("overflow6")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                      # overflow in J^T J is the case
        cost, _, A, B, grad = pr.linearize(g)
        assert np.isfinite(cost) and np.isfinite(grad).all() and np.isfinite(A).all() and np.isfinite(B).all() and 4.4e298 < cost < 4.5e298
        # what overflows is the square of the gradient's norm (entries near 1e298): |r_0| <= eta |g| reads inf <= inf, the linear solve
        # returns x = 0 in 0 iterations, and a zero step has no model decrease
        assert np.abs(grad).max() > 1e290 and np.isinf(grad @ grad)
        s = pr.solve(g, pr.TIGHT)
    assert s["pcg_iterations"] == 0 and all(r[3] == 0 for r in s["trace"])
    assert s["termination"] == 2 and s["num_iterations"] == 5 and s["num_successful_steps"] == 0
    assert _kinds(s["trace"]) == (0,) * 5 and tuple(r[0] for r in s["trace"]) == pr.OVERFLOW_RADII
    assert (s["t"] == g.t).all()


@pytest.mark.parametrize("name", sorted(pr.REPLAY_CASES))
def test_premises_of_the_replayed_steps(name):
    """no decision of a replayed step is within 1e-6 (relative) of its threshold: the device, which differs from the restatement by
    rounding, must take the same one"""
    steps = pr.replay_case(name)
    assert len(steps) == pr.REPLAY_CASES[name][2]
    for k, st in enumerate(steps):
        print(f"{name} step {k}: radius {st['radius']:.6g} reuse {st['reuse']} kind {st['kind']} pcg {st['pcg_iterations']} margins "
              f"pcg {st['pcg_margin']:.2e} rho {st['rho_margin']:.2e} ftol {st['ftol_margin']:.2e} ptol {st['ptol_margin']:.2e}")
        assert min(st["pcg_margin"], st["rho_margin"], st["ftol_margin"], st["ptol_margin"]) > pr.PREMISE, (name, k)
        assert st["kind"] in (1, 2)
    if name == "ring24_far":
        assert tuple(st["kind"] for st in steps[:12]) == pr.FAR_KINDS
    if name == "ring24_far2":
        assert tuple(st["kind"] for st in steps[:6]) == pr.FAR2_KINDS
    # the replay is the prefix of the whole solve
    if name in pr.SOLVE_CASES:
        whole = pr.solve_case(name)["steps"]
        assert all(a["radius"] == b["radius"] and a["kind"] == b["kind"] and (a["x"] == b["x"]).all() for a, b in zip(steps, whole))


def test_trial_step_restates_the_loop():
    """trial_step() in float64 at the restatement's own step gives what solve() computed from it: the verdict on its record is the kind the
    loop logged, and its model change and candidate cost are the trace's to rounding"""
    for name in ("ring24_far", "ring24_ptol"):
        s = pr.solve_case(name)
        g = pr.graph(pr.SOLVE_CASES[name][0])
        for k, (st, row) in enumerate(zip(s["steps"][:16], s["trace"])):
            o = pr.trial_step(g, st["q"], st["t"], st["x"], dtype=np.float64)
            rec = dict(o, finite=1, pcg_iterations=st["pcg_iterations"])
            kind, change, rho = pr.verdict(rec, st["cost"], pr.SOLVE_CASES[name][1])
            assert kind == st["kind"] == int(row[1]), (name, k)
            assert abs(o["model_cost_change"] - row[3]) <= 1e-9 * abs(row[3]) and abs(o["cand_cost"] - row[5]) <= 1e-12 * row[5]
            assert abs(rho - row[4]) <= 1e-9 * abs(row[4])
            assert pr.trace_row(rec, st["radius"], st["cost"], pr.SOLVE_CASES[name][1])[:2] == [row[0], float(row[1])]


def test_trial_step_ignores_fixed_nodes_and_takes_the_old_rotation():
    g = pr.graph("two_fixed")
    q = np.array([pr.quat_from_R(R) for R in g.R])
    x = np.zeros(6 * g.N); x[:6] = 1.0; x[18:24] = -2.0                     # nodes 0 and 3 are fixed
    x[6:12] = [0.3, -0.2, 0.1, 1.0, 2.0, 3.0]
    o = pr.trial_step(g, q, g.t, x)
    assert (o["cand_q"][[0, 3]] == q[[0, 3]]).all() and (o["cand_t"][[0, 3]] == g.t[[0, 3]]).all()
    want_t = g.t[1] + g.R[1] @ x[9:12]
    assert np.abs(np.asarray(o["cand_t"][1], np.float64) - want_t).max() <= 1e-14
    want_R = g.R[1] @ pr.rodrigues(x[6:9])
    assert np.abs(pr.R_from_quat(np.asarray(o["cand_q"][1], np.float64)) - want_R).max() <= 1e-14
    y = x.copy(); y[:6] = 0; y[18:24] = 0
    o2 = pr.trial_step(g, q, g.t, y)
    assert o["model_cost_change"] == o2["model_cost_change"] and o["step2"] == o2["step2"] and o["x2"] == o2["x2"]


def test_measured_pcg_constants_of_the_second_trip_graph():
    """PCG_X_MEASURED's measurement (tests/test_pose_graph_cpu.py::test_measured_constants) on the systems of SECOND_TRIP_PCG_CASES"""
    for name, radius in pr.SECOND_TRIP_PCG_CASES:
        g = pr.graph(name)
        _, _, A, B, grad = pr.linearize(g)
        J = pr.dense_jacobian(g, A, B); H = J.T @ J
        D = pr.lm_diagonal(H, g.fixed)
        x, it, rn, gn = pr.pcg(H, D, radius, grad, g.fixed, 1e-12, pr.PCG_TIGHT_MAX_IT)
        free = np.repeat(g.fixed == 0, 6)
        want = np.zeros_like(x)
        want[free] = np.linalg.solve((H + np.diag(D / radius))[np.ix_(free, free)], -grad[free])
        d = float(np.linalg.norm(x - want) / np.linalg.norm(want))
        print(f"pcg {name} radius {radius}: {it} iterations, |r|/|g| {rn / gn:.2e}, |x - solve| / |solve| {d:.3e}")
        assert it < pr.PCG_TIGHT_MAX_IT and rn <= 1e-12 * gn
        assert 0 < d <= pr.pcg_x_measured(name, radius)
        x1, it1, rn1, gn1 = pr.pcg(H, D, radius, grad, g.fixed, 0.1, 1000)
        assert 1 <= it1 < 1000 and rn1 <= 0.1 * gn1


def test_measured_step_constants():
    assert np.finfo(np.longdouble).nmant >= 63, "numpy.longdouble has no wider mantissa than float64 here: nothing is measured"
    trial, pcgs = 0.0, {}
    for name in sorted(pr.REPLAY_CASES):
        g = pr.graph(pr.REPLAY_CASES[name][0])
        worst = 0.0
        for k, st in enumerate(pr.replay_case(name)):
            want = pr.trial_step(g, st["q"], st["t"], st["x"])
            got = pr.trial_step(g, st["q"], st["t"], st["x"], dtype=np.float64)
            d, parts = pr.trial_distance(g, got, want)
            trial = max(trial, d)
            xl = pr.pcg_k(g, st["A"], st["B"], st["D"], st["radius"], st["grad"], st["pcg_iterations"])
            dx = pr.pcg_distance(st["x"], xl)
            worst = max(worst, dx)
            print(f"{name} step {k}: trial {d:.3e} ({max(parts, key=parts.get)})  pcg ({st['pcg_iterations']} its) {dx:.3e}")
        pcgs[name] = worst
    print(f"TRIAL_MEASURED {trial:.3e}  PCG_STEP_MEASURED {pcgs}")
    assert 0 < trial <= pr.TRIAL_MEASURED
    for name, v in pcgs.items():
        assert 0 < v <= pr.PCG_STEP_MEASURED[name], name
