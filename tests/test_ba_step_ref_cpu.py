"""CPU: the dense one-step reference tests/ba_step_ref.py against the oracle's first Levenberg-Marquardt iteration, the premises of
every case the GPU step tests run, and the MEASUREMENT of the constant those tests are held to.

STEP_MEASURED: for each case and radius the step is solved a second time in plain float64 by eliminating the landmarks
(Step.schur_f64) and its full-system residual |(H_s + D / r) delta + g_s| is evaluated in longdouble against the un-cancelled
magnitude (|H_s| + D / r) |delta| + |g_s|, row by row (Step.residual).  The largest value over all cases of a radius is that radius' constant
in ba_step_ref.py; this file fails if a re-measurement exceeds it.  Blocks come from the oracle's normal_equations() on the CPU."""
import numpy as np
import pytest
import ba_step_ref as bs

ALL = [(n, r) for n, (_, _, radii) in bs.CASES.items() for r in radii]


def _step(oracle, name, radius):
    P = bs.case_premises(name)
    hpp, hll, w, g, cost = oracle.OracleBA(P).normal_equations()
    return P, bs.Step(P, hpp, hll, w, g, P["q"], P["t"], P["X"], radius), cost


@pytest.mark.parametrize("name", list(bs.CASES))
def test_case_premises(name):
    bs.case_premises(name)


@pytest.mark.parametrize("name,radius", ALL, ids=[f"{n} r={r:g}" for n, r in ALL])
def test_measured_constants(oracle, name, radius):
    P, s, _ = _step(oracle, name, radius)
    own = s.residual(s.delta)
    got = s.residual(s.schur_f64())
    print(f"{name} radius {radius:g}: N {s.N} active {len(s.idx)}  reference residual {own:.2e} (last refinement {s.refine_last:.1e})  "
          f"float64 Schur residual {got:.3e}  (STEP_MEASURED {bs.STEP_MEASURED[radius]:.1e})")
    # the refined solution is the reference: its own residual is at longdouble level, far below anything float64 leaves
    assert own <= 1e-18
    assert own < got <= bs.STEP_MEASURED[radius]
    # inactive rows of the reference step are exactly zero, active ones move
    assert not s.delta[~s.act].any() and s.delta[s.act].all()
    # the localising pieces agree with the direct solve: camera rows solve the reduced system, landmark rows follow from them
    red = s.reduced()
    dc = s.delta_s[:6 * s.K].reshape(s.K, 6)[s.slots].reshape(-1)
    assert (np.abs(red["S"] @ dc + red["rhs"]) <= 1e-16 * (red["Smag"] @ np.abs(dc) + red["rhsmag"])).all()
    dl, mag = s.landmark_part(s.delta, red)
    assert (np.abs(dl - s.delta[6 * s.K:].reshape(s.L, 3)) <= 1e-16 * mag).all()


def test_quat_plus_is_the_manifold_update():
    """exp(d) * x on the stored (x, y, z, w): a rotation by |d| about d composed on the left, the norm of x kept; zero step keeps the
    bytes.  Checked against the rotation matrices of the two quaternions."""
    rng = np.random.default_rng(5)

    def R(v):                                   # stored order: v[:3] the vector part, v[3] the scalar
        x, y, z, w = v / np.linalg.norm(v)
        return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                         [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                         [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    for _ in range(20):
        x = rng.normal(size=4) * rng.uniform(0.5, 2); d = rng.normal(size=3) * rng.uniform(1e-3, 1)
        o = bs.quat_plus(x, d)
        th = 2 * np.linalg.norm(d); k = d / np.linalg.norm(d)
        Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        Rd = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
        assert np.abs(R(o) - Rd @ R(x)).max() < 1e-14 and abs(np.linalg.norm(o) - np.linalg.norm(x)) < 1e-15 * 4
        assert (np.abs(o) <= bs.quat_plus_magnitude(x, d) * (1 + 1e-15)).all()
    assert (bs.quat_plus(x, np.zeros(3)) == x).all()


ORACLE_CASES = ["live 5x200", "one free camera 2x60", "16 free of 20", "edges 8x150", "3x257"]


@pytest.mark.parametrize("name", ORACLE_CASES)
def test_reference_reproduces_the_oracles_first_iteration(oracle, name):
    """OracleBA.solve(1)'s trace row against the reference step at radius 1e4: model change, candidate cost (the oracle evaluated at
    the REFERENCE's candidate) and relative decrease.  The oracle's own step is a float64 Schur solve, so it sits within
    10 x STEP_MEASURED[1e4] of the exact one in the residual distance; model_change_slack turns that into a bound on the model change, and
    |g(candidate)| . |A^-1| (rho magnitude) (doubled for the second-order terms) into one on the candidate's cost.  Both also get
    1e-12 relative for their own float64 evaluation."""
    P, s, x_cost = _step(oracle, name, 1e4)
    o = oracle.OracleBA(P)
    o.solve(1)
    row = o.trace()[0]
    assert row[0] == 1e4 and int(row[1]) in (1, 2), row
    rho = 10 * bs.STEP_MEASURED[1e4]
    mc, mag = s.model_change(s.delta)
    slack = s.model_change_slack(s.delta, rho) + 1e-12 * float(mag)
    print(f"{name}: model change oracle {row[3]!r} reference {float(mc)!r} (slack {slack:.2e})")
    assert mc > 0 and abs(row[3] - float(mc)) <= slack
    cq, ct, cX = s.candidate(s.delta)
    Q = dict(P); Q["q"], Q["t"], Q["X"] = cq, ct, cX
    cand_cost, _, _, _, gc = oracle.OracleBA(Q).evaluate()
    e = (np.abs(s.Ainv) @ (rho * s.magnitude(s.delta)).astype(np.float64)) * s.scale[s.idx].astype(np.float64)   # parameter units
    dcost = 2 * float(np.abs(gc[s.idx]) @ e) + 1e-12 * cand_cost
    print(f"{name}: candidate cost oracle {row[5]!r} at the reference's candidate {cand_cost!r} (slack {dcost:.2e})")
    assert abs(row[5] - cand_cost) <= dcost
    assert abs(row[2] - (x_cost - cand_cost)) <= dcost + 1e-12 * x_cost
    rel = (x_cost - cand_cost) / float(mc)
    assert abs(row[4] - rel) <= (dcost + 1e-12 * x_cost + abs(rel) * slack) / float(mc)
    assert (int(row[1]) == 1) == (rel > 1e-3)
    # the accepted candidate is what the oracle holds afterwards, to the same first-order bound
    if int(row[1]) == 1:
        q2, t2, X2 = o.parameters()
        full = np.zeros(s.N); full[s.idx] = e
        lim = 2 * full + 1e-14
        assert (np.abs(t2 - ct).reshape(-1) <= lim[:6 * s.K].reshape(s.K, 6)[:, 3:].reshape(-1)).all()
        assert (np.abs(X2 - cX).reshape(-1) <= lim[6 * s.K:]).all()
