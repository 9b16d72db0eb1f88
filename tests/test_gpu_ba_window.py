"""GPU: dvs_ba_solve_device on windows of 17..63 free cameras (dvs_ba_set_device_window, the tiled solver of csrc/ba.hip) against the
oracle's trust-region loop, the host-Schur solver (dvs_ba_solve) and an independent scipy optimum.  The option is per handle and off
by default: without it every call answers as before.  Tolerances are the ones tests/test_gpu_ba.py states for the in-LDS solver."""
import ctypes as C
import json
import os
import numpy as np
import pytest
from dvslam_amd import synth

pytestmark = pytest.mark.gpu
RTOL = 1e-12
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ITERS = 50

# Parity cases: K straddles the first size the in-LDS solver cannot take (17, 18), crosses n = 192 (33) and reaches the ceiling (64);
# full and partial co-visibility; a second fixed pose with fixed landmarks; the backend's shifted intrinsics (backend.cpp:180).
# Seeds were fixed from the ORACLE alone (CPU), by two conditions: the oracle converges inside ITERS iterations, and its
# (termination, successful steps, iterations) do not move when the inputs are perturbed by 1e-13 and 1e-12 relative (X * (1 + eps),
# uv * (1 - eps)): a run the oracle itself does not repeat under such a perturbation pins no solver.  The plain windows take 5 .. 9
# iterations and pass with their first seed.  The shifted-intrinsics window is the one with rejected steps (24 of its 37 trial
# steps; fx = 10 with sigma = 360 makes the trust region collapse from 1e4 to 1e-7 and candidates fall off the z_c <= 0.1 cut-off):
# seed 34 fails the second condition — the oracle gives (0, 15, 42), (0, 15, 41), (0, 12, 33), (0, 12, 33) for eps = 0, 1e-13, -1e-13,
# 1e-12, and dvs_ba_solve and dvs_ba_solve_device both give (0, 12, 33), agreeing with each other to 1e-8 in every iteration — so the
# next seed that passes it, 35, is used (36 fails too; 37, 39, 41, 44, 47 pass).
# "large noise": the noise levels of tests/ba_bracket.py HARD[1].
CASES = [
    ("17x200", dict(K=17, L=200, seed=17)),
    ("18x200 visibility 0.6", dict(K=18, L=200, seed=18, visibility=0.6)),
    ("24x300", dict(K=24, L=300, seed=5)),
    ("24x250 visibility 0.6, two fixed poses, fixed landmarks", dict(K=24, L=250, seed=6, visibility=0.6, variant="fixed")),
    ("33x300 visibility 0.6", dict(K=33, L=300, seed=33, visibility=0.6)),
    ("33x200 shifted intrinsics", dict(K=33, L=200, seed=35, variant="shifted")),
    ("48x300", dict(K=48, L=300, seed=48)),
    ("20x200 large noise", dict(K=20, L=200, seed=3, pose_noise=(0.2, np.deg2rad(8)), lm_noise=0.3, outlier_frac=0.1)),
    ("64x300 visibility 0.6", dict(K=64, L=300, seed=64, visibility=0.6)),
    ("64x200", dict(K=64, L=200, seed=65)),
]


def make_case(kw):
    kw = dict(kw)
    variant = kw.pop("variant", None)
    P = synth.make_ba_problem(**kw)
    if variant == "fixed":
        P["pose_fixed"][7] = 1
        P["lm_fixed"][::7] = 1
    elif variant == "shifted":                       # (10, fx, fy, cx, sigma = cy), as tests/test_gpu_ba.py builds them
        P["fx"], P["fy"], P["cx"], P["cy"], P["sigma"] = 10.0, 900.0, 900.0, 640.0, 360.0
    return P


def _wide(P):
    from dvslam_amd import BAProblem
    return BAProblem(P).set_device_window(63)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def test_window_of_19_free_cameras_solves_on_the_device(gpu):
    """fails without the feature: there is no set_device_window and solve_device raises DVS_ERR_UNSUPPORTED"""
    g = _wide(synth.make_ba_problem(K=20, L=100, seed=3))
    assert g.device_window() == 63
    s = g.solve_device(5)
    assert s.linear_solver == 1 and s.num_iterations >= 1 and s.final_cost < s.initial_cost


def test_default_is_unchanged(gpu):
    from dvslam_amd import BAProblem, DvsError
    big = synth.make_ba_problem(K=20, L=100, seed=3)
    msg = "dvs_ba_solve_device handles sliding windows (<= 64 cameras, 1..16 of them free); this problem has 20 / 19"
    for g in (BAProblem(big), BAProblem(big).set_device_window(16)):
        assert g.device_window() == 16
        with pytest.raises(DvsError) as e:
            g.solve_device(5)
        assert e.value.code == -2 and msg in str(e.value)
        assert g.solve(5).linear_solver == 2                                  # the host-Schur solver still takes it
    g = BAProblem(big)
    for bad in (0, 64, -1):
        with pytest.raises(DvsError) as e:
            g.set_device_window(bad)
        assert e.value.code == -6                                             # DVS_ERR_ARG
    assert g.device_window() == 16
    g.set_device_window(18)                                                   # a limit below this window's 19 free cameras
    with pytest.raises(DvsError) as e:
        g.solve_device(5)
    assert e.value.code == -2 and "1..18 of them free" in str(e.value)
    g.set_device_window(19)
    assert g.solve_device(5).linear_solver == 1
    with pytest.raises(DvsError) as e:                                        # 65 cameras: the slot table holds 64
        _wide(synth.make_ba_problem(K=65, L=60, seed=2)).solve_device(3)
    assert e.value.code == -2


@pytest.mark.parametrize("name,kw", CASES, ids=[n for n, _ in CASES])
def test_parity_with_oracle_and_host_schur(gpu, oracle, name, kw):
    from dvslam_amd import BAProblem
    P = make_case(kw)
    d = _wide(P); a = BAProblem(P); o = oracle.OracleBA(P)
    sd = d.solve_device(ITERS); sa = a.solve(ITERS); so = o.solve(ITERS)
    key = lambda s: (s.termination, s.num_successful_steps, s.num_iterations)   # noqa: E731
    print(f"{name}: device {key(sd)} host {key(sa)} oracle {key(so)} final {sd.final_cost!r} {sa.final_cost!r} {so.final_cost!r}")
    assert sd.linear_solver == 1 and sa.linear_solver == 2
    assert so.termination == 0 and so.num_iterations < ITERS, "the case must converge inside the cap (fixed from the oracle)"
    assert key(sd) == key(so) and key(sd) == key(sa)
    assert abs(sd.initial_cost - so.initial_cost) <= RTOL * so.initial_cost
    assert abs(sd.final_cost - so.final_cost) <= 1e-6 * so.final_cost, "BA final cost within relative 1e-6 (BASELINE.md §4)"
    assert abs(sd.final_cost - sa.final_cost) <= 1e-9 * sa.final_cost
    q, t, X = d.parameters(); q2, t2, X2 = o.parameters(); qa, ta, Xa = a.parameters()
    assert np.abs(q - q2).max() < 1e-7 and np.abs(q - qa).max() < 1e-7
    assert np.abs(t - t2).max() < 5e-3 and np.abs(X - X2).max() < 5e-2          # loose: the free scale gauge (tests/test_gpu_ba.py)
    for c in np.nonzero(P["pose_fixed"])[0]:
        assert (q[c] == P["q"][c]).all() and (t[c] == P["t"][c]).all()           # gauge pose(s) untouched
    assert (X[P["lm_fixed"] != 0] == P["X"][P["lm_fixed"] != 0]).all()
    assert abs(d.evaluate()[0] - sd.final_cost) <= 1e-12 * sd.final_cost        # the evaluation buffers hold the accepted point


def test_case_set_exercises_the_reject_branch(gpu):
    """at least one parity case rejects a step and goes on (kind 2 in the device solver's own log)"""
    rejected = 0
    for name, kw in CASES:
        if "shifted" in name:
            g = _wide(make_case(kw)); g.solve_device(ITERS)
            rejected += int((g.trace()[:, 1] == 2).sum())
    assert rejected >= 5


def _reduced_system(P, radius=1e4):
    """the Jacobi-scaled, LM-damped reduced camera system of P's first trial step, formed densely in numpy from the Jacobians"""
    from dvslam_amd import BAProblem
    _, r, jp, jl, _ = BAProblem(P).evaluate()
    K, L, R = P["K"], P["L"], len(P["cam_idx"])
    Jp = np.zeros((2 * R, 6 * K)); Jl = np.zeros((2 * R, 3 * L))
    for i in range(R):
        c, l = int(P["cam_idx"][i]), int(P["lm_idx"][i])
        Jp[2 * i:2 * i + 2, 6 * c:6 * c + 6] = jp[i]; Jl[2 * i:2 * i + 2, 3 * l:3 * l + 3] = jl[i]
    free = np.concatenate([np.arange(6 * c, 6 * c + 6) for c in range(K) if not P["pose_fixed"][c]])
    Jp = Jp[:, free]
    sp = 1.0 / (1.0 + np.sqrt((Jp * Jp).sum(0))); sl = 1.0 / (1.0 + np.sqrt((Jl * Jl).sum(0)))
    Jp = Jp * sp; Jl = Jl * sl
    U = Jp.T @ Jp; V = Jl.T @ Jl; W = Jp.T @ Jl
    U += np.diag(np.clip(np.diag(U), 1e-6, 1e32) / radius); V += np.diag(np.clip(np.diag(V), 1e-6, 1e32) / radius)
    Vi = np.linalg.inv(V)
    rr = r.reshape(-1)
    S = U - W @ Vi @ W.T
    rhs = Jp.T @ rr - W @ Vi @ (Jl.T @ rr)
    return np.ascontiguousarray((S + S.T) / 2), np.ascontiguousarray(rhs)


def _probe(hooks, S, rhs):
    from dvslam_amd._lib import check
    n = len(rhs)
    yd = np.zeros(n); xd = np.zeros(n); yh = np.zeros(n); xh = np.zeros(n)
    okd = C.c_int32(); okh = C.c_int32()
    p = lambda a: a.ctypes.data                                                   # noqa: E731
    check(hooks.dvs_ba_factor_probe(0, n, p(S), p(rhs), p(yd), p(xd), p(yh), p(xh), C.byref(okd), C.byref(okh)))
    return yd, xd, yh, xh, okd.value, okh.value


# max |x_tiled - x_host| / max |x_host| over FACTOR_CASES, measured on the MI355X, with a factor 4 of margin for other seeds
STEP_BOUND = 7e-15   # measured 3.0e-16 (n = 102), 6.1e-16 (144), 1.1e-15 (192), 6.2e-16 (288), 1.7e-15 (378): 4 x the largest


FACTOR_CASES = [dict(K=18, L=120, seed=1), dict(K=25, L=150, seed=2, visibility=0.6), dict(K=33, L=150, seed=3), dict(K=49, L=200, seed=4, visibility=0.6),
                dict(K=64, L=200, seed=5)]


@pytest.mark.parametrize("kw", FACTOR_CASES, ids=[f"{k['K']}x{k['L']}" for k in FACTOR_CASES])
def test_tiled_factor_against_chol_solve(gpu, hooks, kw):
    """one linear solve through the tiled launches and through chol_solve on the same S, rhs (hook of the test library only): the
    forward-substituted y — hence the factor — bit-equal; the solution within STEP_BOUND of the host's, relative to its largest
    entry (the backward substitution subtracts from the last unknown down, the host from the first up)."""
    S, rhs = _reduced_system(synth.make_ba_problem(**kw))
    assert len(rhs) == 6 * (kw["K"] - 1)
    yd, xd, yh, xh, okd, okh = _probe(hooks, S, rhs)
    assert okd == 1 and okh == 1
    assert (_bits(yd) == _bits(yh)).all(), f"{int((_bits(yd) != _bits(yh)).sum())} of {len(yd)} entries of y differ"
    err = np.abs(xd - xh).max() / np.abs(xh).max()
    print(f"tiled vs chol_solve, n = {len(rhs)}: max |dx| / max |x| = {err:.3e}")
    assert err <= STEP_BOUND


def test_factor_probe_small_and_indefinite(gpu, hooks):
    """block-column edges (n = 6, 48, 54, 96, 102) and the ceiling on random SPD matrices M M^T, M n x (n + 8) Gaussian, and a matrix
    with a negative pivot: both sides say so.  Bound on x: two backward-stable substitutions differ by ~ cond * n * 2^-53; cond of
    such a matrix is ~ (2 n / 8)^2 < 1e4, so 1e4 * 378 * 1.1e-16 = 4e-10 < 1e-9."""
    rng = np.random.default_rng(7)
    for n in (6, 48, 54, 96, 102, 378):
        M = rng.normal(size=(n, n + 8)); S = np.ascontiguousarray(M @ M.T); rhs = rng.normal(size=n)
        yd, xd, yh, xh, okd, okh = _probe(hooks, S, rhs)
        assert okd == 1 and okh == 1 and (_bits(yd) == _bits(yh)).all(), n
        assert np.abs(xd - xh).max() <= 1e-9 * np.abs(xh).max(), n
    S[200, 200] = -1.0
    *_, okd, okh = _probe(hooks, S, rhs)
    assert okd == 0 and okh == 0


def test_reaches_the_scipy_optimum(gpu):
    """the 24 x 300 window (visibility 0.6) run to convergence lands on the optimum tools/gen_ba_scipy_golden.py found with scipy"""
    z = np.load(os.path.join(GOLD, "ba_scipy_24x300.npz"))
    g = _wide(synth.make_ba_problem(**json.loads(str(z["make_ba_problem_kwargs"]))))
    s = g.solve_device(100, 1e-14, 1e-14, 1e-14)
    assert s.linear_solver == 1
    assert abs(s.initial_cost - float(z["initial_cost"])) <= 1e-9 * s.initial_cost
    assert abs(s.final_cost - float(z["optimum_cost"])) <= 1e-6 * float(z["optimum_cost"]), (s.final_cost, float(z["optimum_cost"]))


def test_two_handles_are_bit_identical(gpu):
    P = synth.make_ba_problem(K=48, L=300, seed=48)
    a = _wide(P); b = _wide(P)
    sa = a.solve_device(ITERS); sb = b.solve_device(ITERS)
    assert (sa.final_cost, sa.num_iterations, sa.num_successful_steps) == (sb.final_cost, sb.num_iterations, sb.num_successful_steps)
    assert (_bits(a.trace()) == _bits(b.trace())).all()
    for x, y in zip(a.parameters(), b.parameters()):
        assert (_bits(x) == _bits(y)).all()


def test_rank_deficient_camera_block(gpu):
    """a camera that sees two landmarks only: its block of the reduced system is singular up to the LM diagonal.  Ordinary arithmetic
    on a rank-deficient input: DVS_OK and the host-Schur solver's termination"""
    from dvslam_amd import BAProblem
    P = synth.make_ba_problem(K=20, L=150, seed=8)
    keep = (P["cam_idx"] != 5) | (P["lm_idx"] < 2)
    for k in ("cam_idx", "lm_idx", "uv"):
        P[k] = np.ascontiguousarray(P[k][keep])
    d = _wide(P); a = BAProblem(P)
    sd = d.solve_device(ITERS); sa = a.solve(ITERS)
    print(f"rank deficient: device {(sd.termination, sd.num_successful_steps, sd.num_iterations)} host {(sa.termination, sa.num_successful_steps, sa.num_iterations)}")
    assert sd.linear_solver == 1 and sd.termination == sa.termination
    assert all(np.isfinite(x).all() for x in d.parameters())


def test_handle_reuse_replans_the_arena(gpu):
    """10 cameras, 40, 10 again on one handle: each solve equals a fresh handle's bit for bit"""
    small = synth.make_ba_problem(K=10, L=400, seed=21); large = synth.make_ba_problem(K=40, L=300, seed=22)
    h = _wide(small)
    for P in (small, large, small):
        h.set_problem(P)
        s = h.solve_device(ITERS)
        f = _wide(P); s2 = f.solve_device(ITERS)
        assert (s.final_cost, s.num_iterations, s.termination) == (s2.final_cost, s2.num_iterations, s2.termination)
        for x, y in zip(h.parameters(), f.parameters()):
            assert (_bits(x) == _bits(y)).all()
    b = _wide(small); b.set_device_window(16)                                     # the setting does not touch windows of <= 16 free cameras
    s3 = b.solve_device(ITERS)
    assert s3.final_cost == s.final_cost


def _same_bits(name, got, want):
    got = got if isinstance(got, (tuple, list)) else (got,)
    want = want if isinstance(want, (tuple, list)) else (want,)
    assert len(got) == len(want), name
    for i, (x, y) in enumerate(zip(got, want)):
        assert np.shape(x) == np.shape(y) and (_bits(x) == _bits(y)).all(), f"{name}[{i}] differs from a fresh handle's"


def _summary(s):
    return [s.termination, s.num_successful_steps, s.num_iterations, s.linear_solver, s.initial_cost, s.final_cost]


def test_one_handle_through_every_entry_point_equals_fresh_handles(gpu):
    """ONE handle through windows of growing and shrinking shape (10x400, 40x300, 3x60, 10x400) with the device window raised and
    lowered in between: evaluate, normal_equations, evaluate_raw, solve and solve_device each give, bit for bit, what a fresh handle
    gives for that window — outputs, summaries, traces and parameters.  (What a stale pointer into a re-planned arena, or a wrong
    boundary between the uploaded, the zero-filled and the output part of an arena, would break.)"""
    from dvslam_amd import BAProblem
    steps = [(dict(K=10, L=400, seed=21), 16), (dict(K=40, L=300, seed=22), 63), (dict(K=3, L=60, seed=23), 63), (dict(K=10, L=400, seed=21), 16)]
    h = None
    for kw, window in steps:
        P = synth.make_ba_problem(**kw)
        if h is None:
            h = BAProblem(P)
        else:
            h.set_device_window(window)
            h.set_problem(P)
        assert h.device_window() == window
        f = BAProblem(P).set_device_window(window)
        for call in ("evaluate", "normal_equations", "evaluate_raw", "evaluate"):     # the second evaluate: after evaluate_raw's buffer exists
            _same_bits(f"{kw} {call}", getattr(h, call)(), getattr(f, call)())
        sh = h.solve(ITERS); sf = f.solve(ITERS)
        _same_bits(f"{kw} solve", _summary(sh) + [h.trace(), *h.parameters()], _summary(sf) + [f.trace(), *f.parameters()])
        assert len(h.trace()) == sh.num_iterations >= 1
        _same_bits(f"{kw} evaluate after solve", h.evaluate(), f.evaluate())
        h.set_problem(P)                                                              # the same shape again: back to the initial point
        f = BAProblem(P).set_device_window(window)
        sh = h.solve_device(ITERS); sf = f.solve_device(ITERS)
        _same_bits(f"{kw} solve_device", _summary(sh) + [h.trace(), *h.parameters()], _summary(sf) + [f.trace(), *f.parameters()])
        assert sh.linear_solver == 1 and len(h.trace()) == sh.num_iterations >= 1
        _same_bits(f"{kw} evaluate after solve_device", h.evaluate(), f.evaluate())
    h.set_device_window(63)                                                           # a new limit alone plans the workspace again
    f = BAProblem(P).set_device_window(63); f.solve_device(ITERS)
    _same_bits("solve_device after a window change", _summary(h.solve_device(ITERS)) + [h.trace(), *h.parameters()],
               _summary(f.solve_device(ITERS)) + [f.trace(), *f.parameters()])
