"""CPU: the reference of one trial step of the global bundle adjustment (tests/gba_step_ref.py): the premises of every case the GPU
step tests run (tests/test_gpu_ba_global_steps.py), the MEASUREMENT of GBA_STEP_MEASURED, and what can and what cannot tell the
model cost change of the step actually taken from a shortcut that assumes an exact solve: no iterate of the PCG can, camera rows
off its Krylov space do.  Blocks come from the oracle's normal_equations() on the CPU."""
import numpy as np
import pytest
import ba_step_ref as bs
import gba_step_ref as gs
import schur_pcg_ref as ref

_BLOCKS = {}


def _blocks(oracle, name):
    if name not in _BLOCKS:
        P = gs.case(name)
        _BLOCKS[name] = (P, oracle.OracleBA(P).normal_equations())
    return _BLOCKS[name]


@pytest.mark.parametrize("name", list(gs.CASES) + ["live 5x200"])
def test_case_premises(name):
    gs.case_premises(name)


@pytest.mark.parametrize("name,radius", gs.MEASURED_AT, ids=[f"{n} r={r:g}" for n, r in gs.MEASURED_AT])
def test_measured_constants(oracle, name, radius):
    P, B = _blocks(oracle, name)
    s = gs.step(P, *B[:4], radius)
    own = s.residual(s.delta)
    its = [gs.pcg_step(P, *B[:4], radius, eta)[2] for eta in (0.1, 1e-6)]
    delta, x, k, rel, ok = gs.pcg_step(P, *B[:4], radius, gs.ETA_EXACT)
    got = s.residual(delta)
    print(f"{name} radius {radius:g}: N {s.N} active {len(s.idx)}  reference residual {own:.2e} (last refinement {s.refine_last:.1e})  "
          f"PCG iterations at eta 0.1 / 1e-6 / 1e-10: {its[0]} / {its[1]} / {k}  recurrence {rel:.2e}  "
          f"residual of the restated step {got:.3e}  (GBA_STEP_MEASURED {gs.GBA_STEP_MEASURED[(name, radius)]:.1e})")
    assert ok == 1 and own <= 1e-18
    assert own < got <= gs.GBA_STEP_MEASURED[(name, radius)]
    assert k < ref.default_cap(int(s.ca.sum())), "the default cap does not end the solve"
    assert not s.delta[~s.act].any() and not delta[~s.act].any()
    # the localising piece agrees with the direct solve: the landmark rows follow from the camera rows
    dl, mag = s.landmark_part(s.delta)
    assert (np.abs(dl - s.delta[6 * s.K:].reshape(s.L, 3)) <= 1e-16 * mag).all()


@pytest.mark.parametrize("name", gs.STRIDES)
def test_what_tells_the_model_change_from_the_exact_solve_shortcut(oracle, name):
    """The premise of the GPU test of "the model cost change is computed from the actual step, so it is right for an inexact one"
    (include/dvslam_hip.h).  The solver's own inexact steps do NOT tell the model cost change of the actual step from the shortcut
    (d.(D / r) d - d.g) / 2 that assumes an exact solve: at ETA_INEXACT the PCG stops far from S x = b (recurrence 0.06), yet the
    two agree to rounding, because a PCG iterate satisfies x.(S x - b) = 0 — at any eta.  Camera rows that are no PCG iterate
    (gba_step_ref.off_krylov_rows of the same iterate, with their own exact back-substitution) do: there the two differ by far
    more than the GPU test allows model_change (1e-11 of its absolute terms), so a kernel that took the shortcut fails on them."""
    P, B = _blocks(oracle, name)
    s = gs.step(P, *B[:4], 1e4)
    S = ref.SchurSystem(P, *B[:4], 1e4)
    x, k, rel, ok = S.pcg(gs.ETA_INEXACT)
    delta = S.back_substitute(x)
    mc, mag = s.model_change(delta)
    short = gs.exact_solve_model_change(s, delta)
    galerkin = abs(x @ (S.S @ x - S.b)) / (np.abs(x) @ (S.Smag @ np.abs(x) + S.bmag))
    d2 = S.back_substitute(gs.off_krylov_rows(x))
    mc2, mag2 = s.model_change(d2)
    short2 = gs.exact_solve_model_change(s, d2)
    print(f"{name}: eta {gs.ETA_INEXACT:g}: {k} iterations, recurrence {rel:.3f}, |x.(S x - b)| {galerkin:.1e} of its terms, model change "
          f"{float(mc)!r}, shortcut {float(short)!r}: {float(abs(mc - short) / mag):.2e} of the absolute terms; off the Krylov space: "
          f"model change {float(mc2)!r}, shortcut {float(short2)!r}: {float(abs(mc2 - short2) / mag2):.2e} (bound of the GPU test 1e-11)")
    assert ok == 1 and mc > 0 and 0.01 < rel <= gs.ETA_INEXACT
    assert galerkin <= 1e-14 and abs(mc - short) <= 1e-13 * mag
    assert mc2 > 0 and abs(mc2 - short2) > 1e3 * 1e-11 * mag2


def test_zero_right_hand_side(oracle):
    """"b = 0": the restatement's b is exactly zero, its PCG returns x = 0 after zero iterations as a VALID solve, the step that
    follows solves the full system (the landmarks move, the cameras do not), and the reference solver makes progress from there"""
    P, B = _blocks(oracle, "b = 0")
    S = ref.SchurSystem(P, *B[:4], 1e4)
    assert not S.b.any()
    x, k, rel, ok = S.pcg(0.1)
    assert (k, rel, ok) == (0, 0.0, 1) and not x.any()
    s = gs.step(P, *B[:4], 1e4)
    delta = S.back_substitute(x)
    assert not delta[:6 * s.K].any() and delta[6 * s.K:].all()
    assert s.residual(delta) <= gs.GBA_STEP_MEASURED[("b = 0", 1e4)]
    assert s.model_change(delta)[0] > 0
    o = oracle.OracleBA(P)
    sm = o.solve(50)
    print(f"b = 0: the oracle takes {sm.num_successful_steps} steps, cost {sm.initial_cost!r} -> {sm.final_cost!r}, termination {sm.termination}")
    assert sm.num_successful_steps >= 1 and sm.final_cost < sm.initial_cost and sm.termination != 2


def test_the_global_active_set_counts_an_unobserved_free_camera():
    """"edges 8x150": the empty free camera is part of the point's norm (xn) under the global rule and not under the window rule"""
    P = gs.case("edges 8x150")
    e = bs.EDGES["empty_cam"]
    ca, la, _ = bs.global_active_blocks(P); wca, wla, _ = bs.active_blocks(P)
    assert (la == wla).all() and ca.sum() == wca.sum() + 1 and ca[e] and not wca[e]
    assert (P["q"][e] ** 2).sum() + (P["t"][e] ** 2).sum() > 0
