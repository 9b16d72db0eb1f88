"""GPU: dvs_pgo_solve (csrc/pose_graph.hip) ONE Levenberg-Marquardt trial step at a time, through dvs_test_pgo_trial_step (test library
only: the three functions the solver's loop is made of — enqueue of a trial, read of its record, commit), against the restatement
tests/pose_graph_ref.py.  A whole run corrects a slightly wrong step and converges anyway; one step does not.

The replay drives the hook with the restatement's radius and reuse flag and commits exactly when the restatement accepts.  The graphs and
what each is for are listed at pose_graph_ref.REPLAY_CASES; tests/test_pose_graph_steps_cpu.py asserts that no decision of a replayed
step is within 1e-6 of its threshold, so equal decisions are demanded here.

Bounds (MARGIN = 10, the factor tests/test_gpu_pose_graph.py gives a kernel that evaluates the same formulas in another order and with
another libm):
* x after k PCG iterations: against pose_graph_ref.pcg_k in longdouble on the DEVICE's system (its blocks and gradient from evaluate(), its
  diagonal from the hook) stopped at the same iteration, |x - x_ld| / |x_ld| <= 10 x PCG_STEP_MEASURED[graph].
* D: clamp(sum of the squared block columns, 1e-6, 1e32) from the device's blocks in longdouble, 1e-13 relative (at most 72 positive
  terms per entry at the hub: 72 eps would be 1.6e-14).
* candidate, cand_cost, model change, step2, x2: against trial_step() in longdouble at the device's x and the poses read back from the
  device, pose_graph_ref.trial_distance <= 10 x TRIAL_MEASURED.
* cur_cost after a commit against the cand_cost before it: 1e-12 relative (two kernels; the margin of the BA step tests)."""
import functools
import numpy as np
import pytest

import pose_graph_ref as pr

pytestmark = pytest.mark.gpu
MARGIN = 10.0
REC = ("cur_cost", "gmax", "cand_cost", "model_cost_change", "step2", "x2", "rnorm", "gnorm", "pcg_iterations", "finite", "breakdown")


def _handle(name, hooks=True):
    from dvslam_amd import PoseGraph
    g = pr.graph(name)
    pg = PoseGraph(hooks=hooks)
    pg.set_nodes(g.R, g.t, g.fixed).set_edges(g.ei, g.ej, g.rvec, g.tvec, g.w_rot, g.w_trans)
    return g, pg


def _drive(gname, params, radii, reuses, commits, with_blocks):
    """the hook through the given steps from the graph's initial poses: per step the hook's dict, the cost of the point as the solver's
    loop carries it (x_cost) and, with_blocks, the device's blocks and gradient at the point (evaluate())"""
    g, pg = _handle(gname)
    out, x_cost = [], None
    for radius, reuse, commit in zip(radii, reuses, commits):
        lin = pg.evaluate() if with_blocks else None
        R_before, t_before = pg.nodes()
        o = pg.trial_step(radius, params["eta"], params["max_pcg_iterations"], reuse_diagonal=reuse, commit=commit)
        if x_cost is None:
            x_cost = o["cur_cost"]
        o.update(x_cost=x_cost, lin=lin, R_before=R_before, t_before=t_before, nodes_after=pg.nodes(), radius=radius)
        out.append(o)
        if commit:
            x_cost = o["cand_cost"]
    pg.close()
    return out


@functools.lru_cache(maxsize=None)
def _replayed(name):
    gname, params, _ = pr.REPLAY_CASES[name]
    steps = pr.replay_case(name)
    return _drive(gname, params, [s["radius"] for s in steps], [s["reuse"] for s in steps], [s["kind"] == 1 for s in steps], True)


@functools.lru_cache(maxsize=None)
def _solved(name):
    gname, params = pr.SOLVE_CASES[name]
    g, pg = _handle(gname, hooks=False)
    s = pg.solve(**params)
    R, t = pg.nodes()
    out = dict(term=s.termination, steps=s.num_successful_steps, its=s.num_iterations, pcg=s.pcg_iterations, final=s.final_cost, initial=s.initial_cost,
               R=R, t=t, trace=pg.trace())
    pg.close()
    return out


@pytest.mark.parametrize("name", sorted(pr.REPLAY_CASES))
def test_step_replay(gpu, hooks, name):
    gname, params, n = pr.REPLAY_CASES[name]
    g = pr.graph(gname)
    ref = pr.replay_case(name)
    dev = _replayed(name)
    assert len(dev) == len(ref) == n
    free6 = np.repeat(g.fixed == 0, 6)
    for k, (st, o) in enumerate(zip(ref, dev)):
        tag = f"{name} step {k}"
        _, _, A, B, grad = o["lin"]
        # the point: a fixed node keeps the poses it was given
        assert o["finite"] == 1 and o["breakdown"] == 0
        assert o["pcg_iterations"] == st["pcg_iterations"], tag
        # ---- the LM diagonal and the step of the linear solve
        AL, BL = A.astype(np.longdouble), B.astype(np.longdouble)
        diag = np.zeros((g.N, 6), np.longdouble)
        np.add.at(diag, g.ei, (AL * AL).sum(1)); np.add.at(diag, g.ej, (BL * BL).sum(1))
        wantD = np.clip(diag.ravel(), 1e-6, 1e32) * free6
        assert (np.abs(o["D"] - wantD) <= 1e-13 * wantD).all(), tag
        xl = pr.pcg_k(g, A, B, o["D"], st["radius"], grad, st["pcg_iterations"])
        dx = pr.pcg_distance(o["x"], xl)
        assert not o["x"][~free6].any()
        # ---- the trial, at the device's own step and point
        want = pr.trial_step(g, o["q"], o["t"], o["x"])
        d, parts = pr.trial_distance(g, o, want)
        kind, change, rho = pr.verdict(o, o["x_cost"], params)
        print(f"{tag}: radius {st['radius']:.6g} reuse {st['reuse']} pcg {o['pcg_iterations']} kind {kind} rho {rho:.4g} (ref {st['rho']:.4g})  "
              f"x {dx:.2e} (bound {MARGIN * pr.PCG_STEP_MEASURED[name]:.1e})  trial {d:.2e} in {max(parts, key=parts.get)} (bound {MARGIN * pr.TRIAL_MEASURED:.1e})")
        assert dx <= MARGIN * pr.PCG_STEP_MEASURED[name], tag
        assert d <= MARGIN * pr.TRIAL_MEASURED, (tag, parts)
        assert kind == st["kind"], tag
        fx = g.fixed != 0
        assert (o["cand_q"][fx] == o["q"][fx]).all() and (o["cand_t"][fx] == o["t"][fx]).all()
        # the record's cost of the point is the cost the loop carries (the cand_cost of the last accepted step), from another kernel
        assert abs(o["cur_cost"] - o["x_cost"]) <= 1e-12 * o["x_cost"], tag
        R_after, t_after = o["nodes_after"]
        if kind == 1:
            assert t_after.tobytes() == o["cand_t"].tobytes()
            assert np.abs(R_after - np.array([pr.R_from_quat(q) for q in o["cand_q"]])).max() <= 4 * np.finfo(np.float64).eps
        else:
            assert R_after.tobytes() == o["R_before"].tobytes() and t_after.tobytes() == o["t_before"].tobytes(), tag
        if k + 1 < n:
            nxt = dev[k + 1]
            if kind == 1:
                assert nxt["q"].tobytes() == o["cand_q"].tobytes() and nxt["t"].tobytes() == o["cand_t"].tobytes()
                assert abs(nxt["cur_cost"] - o["cand_cost"]) <= 1e-12 * o["cand_cost"], tag
            else:      # a rejected step leaves the point, its linearisation and the diagonal as they were
                assert nxt["q"].tobytes() == o["q"].tobytes() and nxt["t"].tobytes() == o["t"].tobytes(), tag
                assert nxt["D"].tobytes() == o["D"].tobytes(), tag
                assert nxt["cur_cost"] == o["cur_cost"] and nxt["gmax"] == o["gmax"]
                assert all(a.tobytes() == b.tobytes() for a, b in zip(nxt["lin"][1:], o["lin"][1:]))
    kinds = [pr.verdict(o, o["x_cost"], params)[0] for o in dev]
    if name == "ring24_far":
        assert tuple(kinds[:12]) == pr.FAR_KINDS
    if name == "ring24_far2":
        assert tuple(kinds[:6]) == pr.FAR2_KINDS


@pytest.mark.parametrize("name", sorted(pr.SOLVE_CASES))
def test_whole_solve_follows_the_restatement_and_the_hook(gpu, hooks, name):
    gname, params = pr.SOLVE_CASES[name]
    ref = pr.solve_case(name)
    s = _solved(name)
    tr = s["trace"]
    n = pr.REPLAY_CASES[name][2] if name in pr.REPLAY_CASES else len(ref["trace"])
    want = np.array(ref["trace"][:n])
    print(f"{name}: termination {s['term']} (ref {ref['termination']}), {s['steps']} / {s['its']} steps (ref {ref['num_successful_steps']} / {ref['num_iterations']}), "
          f"cost {s['final']!r} (ref {ref['final_cost']!r}); kinds {tr[:n, 1].astype(int).tolist()}")
    assert len(tr) >= n
    assert (tr[:n, 1] == want[:, 1]).all() and (tr[:n, 6] == want[:, 6]).all()
    assert (np.abs(tr[:n, 0] - want[:, 0]) <= 1e-9 * want[:, 0]).all()
    if name in ("chain515", "ring24_ptol"):
        assert (s["term"], s["its"], s["steps"]) == (ref["termination"], ref["num_iterations"], ref["num_successful_steps"])
        assert (tr[:, 1] == np.array(ref["trace"])[:, 1]).all()
        assert abs(s["final"] - ref["final_cost"]) <= 1e-6 * ref["final_cost"]
    if name == "ring24_ptol":
        assert tr[-1, 1] == 3 and s["term"] == 0
    if name == "ring24_far2":
        assert s["term"] == 1 and s["its"] == 100
    # the solver's own rows, bit for bit, from the hook driven with the solver's radii, its reuse rule and its accepts
    radii, kinds = tr[:n, 0].tolist(), tr[:n, 1].astype(int).tolist()
    reuses = [False] + [k == 2 for k in kinds[:-1]]
    dev = _drive(gname, params, radii, reuses, [k == 1 for k in kinds], False)
    rows = np.array([pr.trace_row(o, o["radius"], o["x_cost"], params) for o in dev])
    assert rows.tobytes() == tr[:n].tobytes(), np.argwhere(rows != tr[:n])


def test_failure_after_five_invalid_steps(gpu):
    g, pg = _handle("overflow6", hooks=False)
    R0, t0 = pg.nodes()
    s = pg.solve(**pr.TIGHT)
    R, t = pg.nodes()
    tr = pg.trace()
    print(f"overflow6: termination {s.termination}, {s.num_iterations} iterations, rows {tr[:, :2].tolist()}, initial cost {s.initial_cost!r}")
    assert s.termination == 2 and s.num_iterations == 5 and s.num_successful_steps == 0
    assert tr.shape == (5, 7) and (tr[:, 1] == 0).all() and tuple(tr[:, 0]) == pr.OVERFLOW_RADII
    assert R.tobytes() == R0.tobytes() and t.tobytes() == t0.tobytes()
    assert s.final_cost == s.initial_cost and np.isfinite(s.initial_cost)
    # the handle is usable afterwards
    g2 = pr.graph("two_fixed")
    pg.set_nodes(g2.R, g2.t, g2.fixed).set_edges(g2.ei, g2.ej, g2.rvec, g2.tvec, g2.w_rot, g2.w_trans)
    s2 = pg.solve(**pr.TIGHT)
    pg.close()
    assert s2.termination == 0 and abs(s2.final_cost - pr.SCIPY_COST["two_fixed"]) <= 1e-6 * pr.SCIPY_COST["two_fixed"]


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


# rotation part of node 2's step: exactly 0; 1e-160, whose squares are subnormal; 1e-170, whose squares are 0, so that th == 0 from a step
# that is not; 1e-9; 3.0; 7.0, beyond 2 pi
GIVEN = {"zero": 0.0, "underflow": 1e-160, "flushed": 1e-170, "tiny": 1e-9, "three": 3.0, "seven": 7.0}


@pytest.mark.parametrize("case", sorted(GIVEN) + ["fixed", "nan"])
def test_candidate_from_a_given_step(gpu, hooks, case):
    """the candidate and trial kernels alone, on a step the test gives (the linear solve is not launched)"""
    g, pg = _handle("two_fixed")                                              # nodes 0 and 3 are fixed
    x = np.random.default_rng(21).normal(0, 0.05, 6 * g.N)
    x[:6] = 0; x[18:24] = 0
    if case in GIVEN:
        x[12:15] = GIVEN[case] * _unit([0.6, -0.48, 0.64]); x[15:18] = [0.3, -0.2, 0.1]
    if case == "fixed":
        x[:6] = [0.5, -0.4, 0.3, 1.0, 2.0, 3.0]; x[18:24] = -1.0
    if case == "nan":
        x[8] = np.nan
    o = pg.trial_step(1e4, x_in=x)
    pg.close()
    assert o["x"].tobytes() == x.tobytes() and o["pcg_iterations"] == 0 and o["rnorm"] == 0
    fx = g.fixed != 0
    assert o["cand_q"][fx].tobytes() == o["q"][fx].tobytes() and o["cand_t"][fx].tobytes() == o["t"][fx].tobytes()
    if case == "nan":
        assert o["finite"] == 0
        return
    assert o["finite"] == 1
    want = pr.trial_step(g, o["q"], o["t"], x)
    d, parts = pr.trial_distance(g, o, want)
    print(f"{case}: trial distance {d:.2e} in {max(parts, key=parts.get)} (bound {MARGIN * pr.TRIAL_MEASURED:.1e}); model change {o['model_cost_change']:.6g}")
    assert d <= MARGIN * pr.TRIAL_MEASURED, parts
    if case in ("zero", "underflow", "flushed"):                                       # exp of a zero rotation is the identity: the quaternion keeps its bytes up to the renormalisation
        assert np.abs(o["cand_q"][2] - o["q"][2]).max() <= 2 * np.finfo(np.float64).eps
        assert (o["cand_t"][2] != o["t"][2]).all()
    if case == "seven":                                                        # beyond 2 pi: the rotation of 7 - 2 pi about the same axis, the quaternion's sign flipped
        Rw = pr.R_from_quat(o["q"][2]) @ pr.rodrigues((7.0 - 2 * np.pi) * _unit([0.6, -0.48, 0.64]))
        assert np.abs(pr.R_from_quat(o["cand_q"][2]) - Rw).max() <= 1e-14


def test_a_fixed_node_inside_the_second_trip(gpu, hooks):
    """chain515 with node 513 fixed: one whole trial (the linear solve included) where the last trip of the 512-thread loops holds a fixed
    node.  The iteration count is the device's own here (no premise covers this graph); x is held to pcg_k at that count."""
    g, pg = _handle("chain515_fixed")
    lin = pg.evaluate()
    o = pg.trial_step(1e4)
    pg.close()
    assert o["finite"] == 1 and o["breakdown"] == 0 and 1 <= o["pcg_iterations"] < 100 and o["rnorm"] <= 0.1 * o["gnorm"]
    assert not o["x"][6 * 513:6 * 514].any() and not o["D"][6 * 513:6 * 514].any() and not o["x"][:6].any()
    assert o["cand_q"][513].tobytes() == o["q"][513].tobytes() and o["cand_t"][513].tobytes() == o["t"][513].tobytes()
    dx = pr.pcg_distance(o["x"], pr.pcg_k(g, lin[2], lin[3], o["D"], 1e4, lin[4], o["pcg_iterations"]))
    d, parts = pr.trial_distance(g, o, pr.trial_step(g, o["q"], o["t"], o["x"]))
    print(f"chain515_fixed: pcg {o['pcg_iterations']}, x {dx:.2e}, trial {d:.2e} in {max(parts, key=parts.get)}")
    assert dx <= MARGIN * pr.PCG_STEP_MEASURED["chain515"] and d <= MARGIN * pr.TRIAL_MEASURED, parts
    assert pr.verdict(o, o["cur_cost"], pr.TIGHT)[0] == 1


def test_repeatability_with_rejections(gpu):
    first = _solved("ring24_far")
    g, pg = _handle("ring24_far", hooks=False)
    s = pg.solve(**pr.TIGHT)
    R, t = pg.nodes()
    tr = pg.trace()
    assert R.tobytes() == first["R"].tobytes() and t.tobytes() == first["t"].tobytes() and tr.tobytes() == first["trace"].tobytes()
    assert (tr[:, 1] == 2).sum() == (first["trace"][:, 1] == 2).sum() >= 5
    # the same handle: another graph of the same node count in between, then the first again
    g0 = pr.graph("ring24")
    pg.set_nodes(g0.R, g0.t, g0.fixed)
    s0 = pg.solve(**pr.TIGHT)
    assert abs(s0.final_cost - pr.SCIPY_COST["ring24"]) <= 1e-6 * s0.final_cost
    pg.set_nodes(g.R, g.t, g.fixed)
    s1 = pg.solve(**pr.TIGHT)
    R1, t1 = pg.nodes()
    tr1 = pg.trace()
    pg.close()
    assert R1.tobytes() == R.tobytes() and t1.tobytes() == t.tobytes() and tr1.tobytes() == tr.tobytes()
    assert (s1.final_cost, s1.num_iterations, s1.num_successful_steps, s1.pcg_iterations) == (s.final_cost, s.num_iterations, s.num_successful_steps, s.pcg_iterations)
