"""Pose-graph optimisation on the GPU (csrc/pose_graph.hip, dvs_pgo_*) against the float64 restatement tests/pose_graph_ref.py.

Bounds.  evaluate and the operator hook are held to 10 x LIN_MEASURED in the distance pose_graph_ref.lin_distance states — LIN_MEASURED is
how far the restatement in float64 is from the same formulas in numpy.longdouble (measured by tests/test_pose_graph_cpu.py); the factor
10 is the margin the RANSAC stage tests give a kernel that evaluates the same formulas in another order and with another libm.  The
restatement is evaluated at the poses READ BACK from the handle (its R is made from the quaternion), so the comparison has the same
inputs on both sides.  The linear-solve hook is checked against its own stopping rule in float64 and, at eta = 1e-12, against
numpy.linalg.solve within 10 x PCG_X_MEASURED; solves against scipy's recorded cost within 1e-6 relative on both sides (the bracket the BA
tests use) and, on the noise-free graph, against the planted poses within 10 x EXACT_POSE_MEASURED.
evaluate and the two hooks also run on `chain515` (515 nodes, 517 edges: the 512-thread single-workgroup loops make a second trip); its
linear systems carry PCG_X_MEASURED's of their own (pose_graph_ref.PCG_X_MEASURED_SECOND_TRIP, measured in the same way)."""
import functools
import numpy as np
import pytest

import pose_graph_ref as pr

pytestmark = pytest.mark.gpu
MARGIN = 10.0


def _handle(name, hooks=False):
    from dvslam_amd import PoseGraph
    g = pr.graph(name)
    pg = PoseGraph(hooks=hooks)
    pg.set_nodes(g.R, g.t, g.fixed).set_edges(g.ei, g.ej, g.rvec, g.tvec, g.w_rot, g.w_trans)
    return g, pg


@functools.lru_cache(maxsize=None)
def _solved(name):
    """(graph, summary fields, R, t, trace, poses before the solve) of one solve with the tight tolerances, shared by the tests"""
    g, pg = _handle(name)
    R0, t0 = pg.nodes()
    s = pg.solve(**pr.TIGHT)
    R, t = pg.nodes()
    out = dict(g=g, term=s.termination, steps=s.num_successful_steps, its=s.num_iterations, pcg=s.pcg_iterations, initial=s.initial_cost,
               final=s.final_cost, R=R, t=t, trace=pg.trace(), R0=R0, t0=t0)
    pg.close()
    return out


def _fixed_rows(g):
    return np.repeat(g.fixed != 0, 6)


@pytest.mark.parametrize("name", pr.ALL_GRAPHS + pr.SECOND_TRIP_GRAPHS)
def test_evaluate(gpu, name):
    g, pg = _handle(name)
    R, t = pg.nodes()
    got = pg.evaluate()
    pg.close()
    # R -> quaternion -> R: every entry (at most 1) is a handful of products of components that each carry a few ulp (Shepperd's root and
    # division, the normalisation): 32 ulp of 1
    assert np.abs(R - g.R).max() <= 32 * np.finfo(np.float64).eps and (t == g.t).all()
    want = pr.linearize(g, R, t, dtype=np.longdouble)
    d = pr.lin_distance(g, got, want)
    print(f"{name}: distance {d:.3e} (bound {MARGIN * pr.LIN_MEASURED:.1e})")
    assert all(np.isfinite(x).all() for x in got)
    assert d <= MARGIN * pr.LIN_MEASURED
    # rows of fixed nodes: exactly zero, in the gradient and in the blocks
    assert not got[4][_fixed_rows(g)].any()
    assert not got[2][g.fixed[g.ei] != 0].any() and not got[3][g.fixed[g.ej] != 0].any()
    if name == "zero_rot":
        assert not got[1][-1, :3].any()                                        # Log of the identity is the zero vector, not NaN
    if name == "tiny_rot":
        assert 0.5e-9 * 300 < np.linalg.norm(got[1][-1, :3]) < 2e-9 * 300
    if name == "big_rot":
        assert abs(np.linalg.norm(got[1][-1, :3]) / 300 - 3.0) < 1e-6
    if name == "isolated":
        assert not got[4][36:42].any()


def _operator(g, A, B, radius, p):
    """(H + D / radius) p over the free rows in longdouble, from the GPU's own blocks: J p per edge, J^T of that per node"""
    J = pr.dense_jacobian(g, A.astype(np.longdouble), B.astype(np.longdouble))
    free = ~_fixed_rows(g)
    D = np.clip((J * J).sum(0), 1e-6, 1e32) * free
    y = J.T @ (J @ (p * free)) + D * p / radius
    return np.where(free, y, 0), J, D


@pytest.mark.parametrize("name,radius", [("ring24", 1e4), ("hub300", 1e4), ("hub300", 0.5), ("two_fixed", 3.0), ("chain515", 1e4), ("chain515", 1.0),
                                         ("chain515_fixed", 1.0)])
def test_apply_hook(gpu, hooks, name, radius):
    g, pg = _handle(name, hooks=True)
    _, _, A, B, _ = pg.evaluate()
    p = np.random.default_rng(8).normal(size=6 * g.N)
    y = pg.apply(radius, p)
    pg.close()
    want, J, D = _operator(g, A, B, radius, p.astype(np.longdouble))
    # the distance of lin_distance for this quantity: against its largest magnitude, which no cancellation undercuts (random p)
    d = float(np.abs(y - want).max() / np.abs(want).max())
    print(f"{name} radius {radius}: distance {d:.3e}")
    assert d <= MARGIN * pr.LIN_MEASURED
    assert not y[_fixed_rows(g)].any()
    if g.N > 512:
        # the single-workgroup loops' second trip alone: p is zero except in nodes 512 .., so only those rows and their neighbours' are not zero
        g, pg = _handle(name, hooks=True)
        p2 = np.zeros_like(p); p2[6 * 512:] = p[6 * 512:]
        y2 = pg.apply(radius, p2)
        pg.close()
        want2 = _operator(g, A, B, radius, p2.astype(np.longdouble))[0]
        near = np.zeros(g.N, bool); near[512:] = True
        for i, j in zip(g.ei, g.ej):
            if i >= 512 or j >= 512:
                near[[i, j]] = True
        rows = np.repeat(near, 6)
        assert near.sum() > g.N - 512 and (want2[np.repeat(near & (g.fixed == 0), 6)] != 0).all()
        assert np.abs(y2 - want2)[rows].max() <= MARGIN * pr.LIN_MEASURED * float(np.abs(want2).max())
        assert not y2[~rows].any() and not y2[_fixed_rows(g)].any()


@pytest.mark.parametrize("name,radius", pr.PCG_CASES + pr.SECOND_TRIP_PCG_CASES)
def test_pcg_hook(gpu, hooks, name, radius):
    g, pg = _handle(name, hooks=True)
    _, _, A, B, grad = pg.evaluate()
    free = ~_fixed_rows(g)
    gl = grad.astype(np.longdouble)

    def true_residual(x):
        return float(np.sqrt(((_operator(g, A, B, radius, x.astype(np.longdouble))[0] + gl * free) ** 2).sum()))
    gnorm = float(np.sqrt((gl * gl * free).sum()))
    x, it, rn, gn = pg.pcg(radius, 0.1, 1000)
    assert 1 <= it < 1000 and abs(gn - gnorm) <= 1e-12 * gnorm and not x[~free].any()
    r_true = true_residual(x)
    print(f"{name} radius {radius}: eta 0.1 stops after {it} iterations, |Ax + g| / |g| = {r_true / gnorm:.4f}, recurrence {rn / gn:.4f}")
    assert r_true <= 0.1 * gnorm * (1 + 1e-9) and rn <= 0.1 * gn
    x_prev, it_prev, rn_prev, _ = pg.pcg(radius, 0.1, it - 1)                 # one iteration earlier the condition does not hold yet
    assert it_prev == it - 1 and true_residual(x_prev) > 0.1 * gnorm and rn_prev > 0.1 * gn
    xz, itz, _, _ = pg.pcg(radius, 0.1, 0)
    assert itz == 0 and not xz.any()
    xt, itt, rnt, _ = pg.pcg(radius, 1e-12, pr.PCG_TIGHT_MAX_IT)
    pg.close()
    J = pr.dense_jacobian(g, A, B)
    Am = (J.T @ J + np.diag(np.asarray(_operator(g, A, B, radius, np.zeros(6 * g.N, np.longdouble))[2], np.float64) / radius))[np.ix_(free, free)]
    want = np.zeros(6 * g.N); want[free] = np.linalg.solve(Am, -grad[free])
    d = float(np.linalg.norm(xt - want) / np.linalg.norm(want))
    measured = pr.pcg_x_measured(name, radius)
    print(f"{name} radius {radius}: eta 1e-12 stops after {itt} iterations, |x - solve| / |solve| = {d:.3e} (bound {MARGIN * measured:.1e})")
    assert itt < pr.PCG_TIGHT_MAX_IT and rnt <= 1e-12 * gn
    assert d <= MARGIN * measured


@pytest.mark.parametrize("name", ("ring24", "hub300") + pr.EDGE_CASES)
def test_solve_reaches_scipys_cost(gpu, name):
    s = _solved(name)
    want = pr.SCIPY_COST[name]
    print(f"{name}: cost {s['initial']:.6g} -> {s['final']!r} (scipy {want!r}), {s['steps']} / {s['its']} steps, {s['pcg']} PCG iterations")
    assert s["term"] == 0 and s["final"] <= s["initial"]
    assert abs(s["final"] - want) <= 1e-6 * want + pr.ZERO_COST
    g = s["g"]
    # the cost the summary reports is the cost of the poses the handle returns
    again = pr.linearize(g, s["R"], s["t"])[0]
    assert abs(again - s["final"]) <= 1e-9 * again + pr.ZERO_COST
    # rows of the trace: the PCG column sums to the summary's total, accepted rows to its successful steps
    tr = s["trace"]
    assert tr.shape == (s["its"], 7) and tr[:, 6].sum() == s["pcg"] and (tr[:, 1] == 1).sum() == s["steps"]
    # fixed nodes keep their bytes; so does an isolated free node (zero gradient, zero step)
    keep = np.flatnonzero(g.fixed)
    assert (s["R"][keep] == s["R0"][keep]).all() and (s["t"][keep] == s["t0"][keep]).all()
    if name == "isolated":
        assert (s["R"][6] == s["R0"][6]).all() and (s["t"][6] == s["t0"][6]).all()
    assert np.abs(s["R"] @ s["R"].transpose(0, 2, 1) - np.eye(3)).max() <= 1e-14   # the quaternion is renormalised


def test_solve_recovers_the_planted_poses(gpu):
    s = _solved("exact24")
    R, t = s["g"].planted
    d = max(np.abs(s["R"] - R).max(), np.abs(s["t"] - t).max())
    print(f"exact24: cost {s['initial']:.6g} -> {s['final']:.3e}, |pose - planted| {d:.3e} (bound {MARGIN * pr.EXACT_POSE_MEASURED:.1e})")
    assert s["term"] == 0 and s["final"] <= pr.ZERO_COST
    assert d <= MARGIN * pr.EXACT_POSE_MEASURED


@pytest.mark.parametrize("name", ("ring24", "hub300"))
def test_two_identical_solves_return_identical_bytes(gpu, name):
    first = _solved(name)
    g, pg = _handle(name)
    s = pg.solve(**pr.TIGHT)
    R, t = pg.nodes()
    assert R.tobytes() == first["R"].tobytes() and t.tobytes() == first["t"].tobytes()
    assert pg.trace().tobytes() == first["trace"].tobytes() and s.final_cost == first["final"] and s.pcg_iterations == first["pcg"]
    # the same handle again from the same start: set_nodes of the same count keeps the edges
    pg.set_nodes(g.R, g.t, g.fixed)
    pg.solve(**pr.TIGHT)
    R2, t2 = pg.nodes()
    pg.close()
    assert R2.tobytes() == R.tobytes() and t2.tobytes() == t.tobytes()


def test_default_parameters_and_iteration_limit(gpu):
    g, pg = _handle("ring24")
    s = pg.solve()
    assert s.termination == 0 and abs(s.final_cost - pr.SCIPY_COST["ring24"]) <= 1e-5 * s.final_cost
    pg.set_nodes(g.R, g.t, g.fixed)
    s = pg.solve(max_iterations=2)
    assert s.termination == 1 and s.num_iterations == 2 and len(pg.trace()) == 2
    pg.set_nodes(g.R, g.t, g.fixed)
    s = pg.solve(max_iterations=0)
    R, t = pg.nodes()
    assert s.termination == 1 and s.initial_cost == s.final_cost and (t == g.t).all()
    pg.close()


def test_correct_points(gpu):
    s = _solved("ring24")
    g, pg = _handle("ring24")
    pg.solve(**pr.TIGHT)
    R1, t1 = pg.nodes()
    assert R1.tobytes() == s["R"].tobytes()
    rng = np.random.default_rng(12)
    n_all, n = 700, 613                                                        # more than two workgroups, not a multiple of 256
    xyz = rng.uniform(-7, 7, (n_all, 3)).astype(np.float32)
    anchor = rng.integers(0, g.N, n_all).astype(np.int32)
    anchor[[5, 300]] = -1; anchor[[6, 301]] = g.N; anchor[7] = np.iinfo(np.int32).max; anchor[8] = np.iinfo(np.int32).min
    got = pg.correct_points(xyz, anchor, n)
    want = pr.correct_points(xyz[:n], anchor[:n], g.R, g.t, R1, t1)
    assert got[:n].tobytes() == want.tobytes()                                 # the ref's float64 sequence, bit for bit
    assert (got[[5, 300, 6, 301, 7, 8]] == xyz[[5, 300, 6, 301, 7, 8]]).all() and (got[n:] == xyz[n:]).all()
    moved = np.abs(got[:n] - xyz[:n]).max()
    assert 1e-3 < moved < 2.0                                                  # the correction is the drift that the loops removed
    # device form on caller memory, rows past n untouched there too
    from dvslam_amd._lib import DeviceBuffer
    dx, da = DeviceBuffer(xyz.nbytes).upload(xyz), DeviceBuffer(anchor.nbytes).upload(anchor)
    pg.correct_points_device(n, dx.ptr, da.ptr)
    pg.synchronize()
    assert dx.download(np.float32, xyz.size).tobytes() == got.tobytes()
    dx.free(); da.free()
    # before any solve "before" and current differ only by R -> quaternion -> R: points come back to float rounding
    g2, pg2 = _handle("ring24")
    same = pg2.correct_points(xyz, anchor)
    pg2.close(); pg.close()
    assert np.abs(same - xyz).max() <= 4e-6


def test_argument_errors_on_a_handle(gpu):
    from dvslam_amd import PoseGraph, DvsError
    g = pr.graph("two_fixed")
    pg = PoseGraph()

    def refused(f, *a):
        with pytest.raises(DvsError) as e:
            f(*a)
        assert e.value.code == -6
    refused(pg.set_edges, g.ei, g.ej, g.rvec, g.tvec, g.w_rot, g.w_trans)      # edges before nodes
    refused(pg.nodes)
    refused(pg.set_nodes, g.R, g.t, np.zeros(g.N, np.uint8))                   # no fixed node
    pg.set_nodes(g.R, g.t, g.fixed)
    refused(pg.solve)                                                          # no edges yet
    bad = g.ej.copy(); bad[2] = g.ei[2]
    refused(pg.set_edges, g.ei, bad, g.rvec, g.tvec, g.w_rot, g.w_trans)
    bad = g.ei.copy(); bad[0] = g.N
    refused(pg.set_edges, bad, g.ej, g.rvec, g.tvec, g.w_rot, g.w_trans)
    w = g.w_rot.copy(); w[1] = 0
    refused(pg.set_edges, g.ei, g.ej, g.rvec, g.tvec, w, g.w_trans)
    rv = g.rvec.copy(); rv[1, 1] = np.nan
    refused(pg.set_edges, g.ei, g.ej, rv, g.tvec, g.w_rot, g.w_trans)
    pg.set_edges(g.ei, g.ej, g.rvec, g.tvec, g.w_rot, g.w_trans)
    refused(lambda: pg.solve(eta=0.0))
    refused(lambda: pg.solve(max_iterations=-1))
    s = pg.solve(**pr.TIGHT)                                                   # the refused calls left the handle usable
    assert abs(s.final_cost - pr.SCIPY_COST["two_fixed"]) <= 1e-6 * s.final_cost
    pg.set_nodes(g.R[:4], g.t[:4], g.fixed[:4])                                # another node count drops the edges
    refused(pg.solve)
    pg.close()
