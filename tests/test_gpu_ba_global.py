"""GPU: dvs_ba_solve_global (csrc/ba.hip) — the camera steps by matrix-free Schur PCG, any number of keyframes — against the dense
numpy restatement of its linear solve (tests/schur_pcg_ref.py), the two existing solvers, and an independent scipy optimum.
The four systems (a)..(d) are schur_pcg_ref.system_problem's: more than 64 cameras, two chunks per camera, landmarks on both sides of
k_lm_backsub's 16-observation path.  The second trip of the loops that stride the cameras by 256, a K that is no multiple of 4 and
the chunk edges (63 / 64 / 65, 256 / 257 observations, three chunks) are tests/test_gpu_ba_global_steps.py's, one trial step at a
time."""
import numpy as np
import pytest
import schur_pcg_ref as ref

pytestmark = pytest.mark.gpu

_PROBLEMS = {}


def problem(name):
    """a fresh copy of system (a)..(d), or "b-edges": (b) with a second fixed camera, every seventh landmark fixed, one landmark with
    no observation left, one with a single observation, one observation duplicated in its camera, and one camera with no observation"""
    if name not in _PROBLEMS:
        if name == "b-edges":
            P = ref.system_problem("b")
            P["pose_fixed"][40] = 1
            P["lm_fixed"][::7] = 1
            cam, lm, uv = P["cam_idx"], P["lm_idx"], P["uv"]
            keep = lm != 5                                                     # landmark 5: nobody sees it any more
            first9 = np.nonzero(lm == 9)[0][0]
            keep &= (lm != 9) | (np.arange(len(lm)) == first9)                 # landmark 9: a single observation
            keep &= cam != 60                                                  # camera 60: no observation
            dup = np.nonzero((lm == 13) & keep)[0][1]                          # an observation of landmark 13, a second time in its camera
            cam = np.concatenate([cam[keep], cam[dup:dup + 1]]); lm = np.concatenate([lm[keep], lm[dup:dup + 1]])
            uv = np.concatenate([uv[keep], uv[dup:dup + 1] + np.array([[0.75, -0.5]])])
            assert not P["lm_fixed"][[5, 9, 13]].any()
            P["cam_idx"], P["lm_idx"], P["uv"] = np.ascontiguousarray(cam), np.ascontiguousarray(lm), np.ascontiguousarray(uv)
        else:
            P = ref.system_problem(name)
        _PROBLEMS[name] = P
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in _PROBLEMS[name].items()}


_DENSE = {}


def dense(name, radius):
    """the dense system of `name` at its initial point, from the DEVICE's Jacobians (as test_gpu_ba_window._reduced_system does)"""
    from dvslam_amd import BAProblem
    if name not in _DENSE:
        P = problem(name)
        _, r, jp, jl, _ = BAProblem(P).evaluate()
        _DENSE[name] = (P, ref.blocks_from_jacobians(P, r, jp, jl))
    if (name, radius) not in _DENSE:
        P, (hpp, hll, w, g) = _DENSE[name]
        _DENSE[(name, radius)] = ref.SchurSystem(P, hpp, hll, w, g, radius)
    return _DENSE[(name, radius)]


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def test_more_than_64_cameras_solve_on_the_device(gpu):
    """fails without the feature: (a) has 96 cameras, dvs_ba_solve_device refuses it and there is no dvs_ba_solve_global"""
    from dvslam_amd import BAProblem, DvsError
    g = BAProblem(problem("a"))
    with pytest.raises(DvsError) as e:
        g.solve_device(5)
    assert e.value.code == -2
    s = g.solve_global()
    assert s.ba.linear_solver == 3 and s.ba.termination == 0 and s.ba.final_cost < s.ba.initial_cost and s.pcg_iterations >= 1
    it, rel = g.pcg_trace()
    assert len(it) == len(g.trace()) == s.ba.num_iterations and it.sum() == s.pcg_iterations and (it >= 1).all()


@pytest.mark.parametrize("radius", [1e4, 1e8])
@pytest.mark.parametrize("name", ["a", "b", "c", "b-edges"])
def test_operator_preconditioner_and_rhs(gpu, hooks, name, radius):
    """dvs_ba_schur_probe against the dense S, M^-1 and b.  Bounds are forward-error bounds, not measurements:
    * S x and b element-wise against the UN-CANCELLED magnitudes, |y - S x| <= 1e-11 (|A| + |B| |C^-1| |B^T|) |x|: 1e-11 is about 5e4
      eps against at most a few thousand summed terms per row;
    * M^-1 by its residual against the dense block: M Minv - I = (M - M_dev) Minv + (M_dev Minv - I), the first term bounded as above
      (1e-11 |M|_uncancelled |Minv|), the second the residual of a 6 x 6 Cholesky inverse, <= 1e-13 cond(M) (some hundred eps)."""
    from dvslam_amd import BAProblem
    s = dense(name, radius)
    P = problem(name)
    g = BAProblem(P, hooks=True)
    K = P["K"]
    free = np.nonzero(s.free)[0]
    rng = np.random.Generator(np.random.PCG64(7))
    xs = [rng.normal(0, 1, 6 * K) for _ in range(3)]
    for c in (free[0], free[-1]):
        e = np.zeros(6 * K); e[6 * c + 2] = 1.0
        xs.append(e)
    worst = 0.0
    for x in xs:
        y, Minv, b = g.schur_probe(radius, x)
        xm = x * np.repeat(s.free, 6)
        bound = 1e-11 * (s.Smag @ np.abs(xm))
        err = np.abs(y - s.S @ xm)
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()) * 1e-11)
        assert (err <= bound).all(), f"{name} radius {radius:g}: |y - S x| up to {worst:.2e} of the un-cancelled magnitude"
        assert (y.reshape(K, 6)[~s.free] == 0).all()
    print(f"{name} radius {radius:g}: |y - S x| <= {worst:.2e} x un-cancelled magnitude")
    assert (np.abs(b - s.b) <= 1e-11 * s.bmag).all()
    assert (b.reshape(K, 6)[~s.free] == 0).all() and (Minv[~s.free] == 0).all()
    for c in free:
        res = np.abs(s.M[c] @ Minv[c] - np.eye(6)).max()
        lim = 1e-11 * np.abs(s.Mmag[c]).sum(1).max() * np.abs(Minv[c]).sum(0).max() + 1e-13 * np.linalg.cond(s.M[c])
        assert res <= lim, f"{name} radius {radius:g} camera {c}: |M Minv - I| = {res:.2e} > {lim:.2e}"
        assert np.abs(Minv[c] - Minv[c].T).max() <= 1e-12 * np.abs(Minv[c]).max()


@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_linear_solve_reaches_its_residual(gpu, hooks, name):
    """one linear solve at eta = 1e-6 and the first trial step's radius: the device's x has true residual <= 2 eta |b| against the
    dense S, and stops within two iterations of the restatement (rounding may move the stopping iteration by one); the solve's own
    first trial step ran exactly that many iterations"""
    from dvslam_amd import BAProblem
    eta = 1e-6
    s = dense(name, 1e4)
    g = BAProblem(problem(name), hooks=True)
    x, it, rel, ok = g.pcg_probe(1e4, eta)
    _, it_ref, rel_ref, _ = s.pcg(eta)
    true = np.linalg.norm(s.S @ x - s.b) / np.linalg.norm(s.b)
    print(f"({name}) device {it} iterations, recurrence {rel:.3e}, true {true:.3e}; restatement {it_ref} iterations, {rel_ref:.3e}")
    assert ok == 1 and rel <= eta
    assert true <= 2 * eta
    assert abs(it - it_ref) <= 2
    sg = g.solve_global(max_iterations=1, eta=eta)
    its, rels = g.pcg_trace()
    assert sg.ba.num_iterations == 1 and len(its) == 1 and its[0] == it and _bits(rels[0]) == _bits(rel)


@pytest.mark.parametrize("name", ["c", "d"])
def test_near_exact_steps_follow_the_direct_solver(gpu, name):
    """eta = 1e-10: the trust-region run is the direct device solver's"""
    from dvslam_amd import BAProblem
    d = BAProblem(problem(name)).set_device_window(63); g = BAProblem(problem(name))
    sd = d.solve_device(50); sg = g.solve_global(eta=1e-10).ba
    key = lambda s: (s.termination, s.num_successful_steps, s.num_iterations)   # noqa: E731
    print(f"({name}) direct {key(sd)} {sd.final_cost!r} global {key(sg)} {sg.final_cost!r} gap {abs(sd.final_cost - sg.final_cost) / sd.final_cost:.2e}")
    assert key(sg) == key(sd)
    assert abs(sg.final_cost - sd.final_cost) <= 1e-9 * sd.final_cost


@pytest.mark.parametrize("name", ["a", "b", "d"])
def test_inexact_steps_reach_the_same_minimum(gpu, name):
    """default eta = 0.1: another path to the minimum the host solver finds with the same tolerances"""
    import ba_bracket as bb
    from dvslam_amd import BAProblem
    h = BAProblem(problem(name)); g = BAProblem(problem(name))
    sh = h.solve(100, 1e-10, 1e-10, 1e-8)
    sg = g.solve_global(max_iterations=100, function_tolerance=1e-10)
    print(f"({name}) host {sh.num_iterations} iterations {sh.final_cost!r}; global {sg.ba.num_iterations} iterations, "
          f"{sg.pcg_iterations} PCG iterations, {sg.ba.final_cost!r}; gap {abs(sg.ba.final_cost - sh.final_cost) / sh.final_cost:.2e}")
    assert sh.termination == 0 and sg.ba.termination == 0
    assert abs(sg.ba.final_cost - sh.final_cost) <= 1e-8 * sh.final_cost
    tr = g.trace()
    bb.check_schedule(tr)
    cost = sg.ba.initial_cost
    for row in tr[tr[:, 1] == 1]:
        assert row[5] < cost
        cost = row[5]
    assert abs(cost - sg.ba.final_cost) <= 1e-12 * cost      # the candidate's cost-only evaluation and the full one differ in the last bit


def test_reaches_the_scipy_optimum(gpu):
    """(b) against the optimum scipy.optimize.least_squares found (tools/gen_ba_scipy_golden.py): cost within 1e-6 relative
    (BASELINE.md §4), poses and landmarks up to the free scale gauge at the tolerances tests/test_gpu_ba.py uses"""
    import ba_bracket as bb
    from dvslam_amd import BAProblem, synth
    kw, G = bb.scipy_golden("80x400_banded")
    assert str(G["generator"]) == "make_ba_banded_problem"
    g = BAProblem(synth.make_ba_banded_problem(**kw))
    s = g.solve_global(max_iterations=100, function_tolerance=1e-10).ba
    gap = abs(s.final_cost - float(G["optimum_cost"])) / float(G["optimum_cost"])
    q, t, X = g.parameters()
    ang, dc, dX, scale = bb.gauge_aligned_errors(q, t, X, G["q"], G["t"], G["X"])
    print(f"scipy optimum {float(G['optimum_cost'])!r}, global {s.final_cost!r}: gap {gap:.2e}; angle {ang:.2e} centre {dc:.2e} landmark {dX:.2e} scale {scale!r}")
    assert abs(s.initial_cost - float(G["initial_cost"])) <= 1e-9 * s.initial_cost
    assert s.termination == 0 and gap <= 1e-6
    assert ang < 2e-4 and dc < 2e-3, (ang, dc, dX, scale)


def test_two_solves_return_identical_bytes(gpu):
    from dvslam_amd import BAProblem
    runs = []
    for _ in range(2):
        g = BAProblem(problem("a"))
        s = g.solve_global(eta=1e-3)
        runs.append((s.ba.final_cost, s.pcg_iterations, g.parameters(), g.trace(), g.pcg_trace()))
    a, b = runs
    assert a[0] == b[0] and a[1] == b[1] and a[1] > len(a[3])
    for x, y in zip(a[2], b[2]):
        assert (_bits(x) == _bits(y)).all()
    assert (_bits(a[3]) == _bits(b[3])).all()
    assert (a[4][0] == b[4][0]).all() and (_bits(a[4][1]) == _bits(b[4][1])).all()


def test_fixed_blocks_and_evaluation_buffers(gpu):
    from dvslam_amd import BAProblem
    P = problem("b-edges")
    g = BAProblem(P)
    s = g.solve_global().ba
    assert s.termination == 0 and s.final_cost < s.initial_cost
    q, t, X = g.parameters()
    for c in (0, 40, 60):                                  # two fixed cameras, and the one without observations
        assert (_bits(q[c]) == _bits(P["q"][c])).all() and (_bits(t[c]) == _bits(P["t"][c])).all()
    still = (P["lm_fixed"] != 0); still[5] = True          # fixed landmarks and the one nobody observes
    assert (_bits(X[still]) == _bits(P["X"][still])).all()
    assert (X[~still] != P["X"][~still]).any(axis=1).all()
    assert abs(g.evaluate()[0] - s.final_cost) <= 1e-12 * s.final_cost


def test_handle_takes_a_smaller_then_a_larger_problem(gpu):
    from dvslam_amd import BAProblem
    fresh = {n: BAProblem(problem(n)).solve_global().ba for n in ("c", "a")}
    g = BAProblem(problem("b"))
    g.solve_global()
    for n in ("c", "a"):
        g.set_problem(problem(n))
        s = g.solve_global().ba
        assert (s.termination, s.num_iterations, s.final_cost) == (fresh[n].termination, fresh[n].num_iterations, fresh[n].final_cost)


def test_arguments_and_unchanged_limits(gpu):
    from dvslam_amd import BAProblem, DvsError, synth
    g = BAProblem(problem("c"))
    for bad in (dict(eta=0.0), dict(eta=1.0), dict(eta=-0.5), dict(eta=float("nan")), dict(max_iterations=-1), dict(max_pcg_iterations=-1),
                dict(function_tolerance=-1e-6)):
        with pytest.raises(DvsError) as e:
            g.solve_global(**bad)
        assert e.value.code == -6, bad
    with pytest.raises(TypeError):
        g.solve_global(etta=0.1)
    P = problem("c"); P["pose_fixed"][:] = 1
    with pytest.raises(DvsError) as e:
        BAProblem(P).solve_global()
    assert e.value.code == -6
    with pytest.raises(DvsError) as e:
        BAProblem(synth.make_ba_problem(K=65, L=60, seed=2)).set_device_window(63).solve_device(3)
    assert e.value.code == -2
    assert "dvs_ba_solve_device handles sliding windows (<= 64 cameras, 1..63 of them free); this problem has 65 / 64" in str(e.value)
    assert g.solve_global(max_pcg_iterations=3, eta=1e-10, max_iterations=2).pcg_iterations == 6     # the cap ends a linear solve
