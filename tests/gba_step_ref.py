"""Reference of ONE trial step of the global bundle adjustment (dvs_ba_solve_global; include/dvslam_hip.h, "Global BA"), and the
problems its step tests use.  numpy only; nothing here follows the kernels.  It stands on the two references the suite has:

* tests/ba_step_ref.py's Step, the dense longdouble solve of the FULL (6K + 3L) system, here with the global solver's active set
  (ba_step_ref.global_active_blocks: every camera that is not fixed is active, observed or not; the window solver also asks for an
  observation).  An inexact camera step is judged in it like an exact one: Step.residual is the row-wise distance of any step from
  solving the full system, Step.landmark_part the landmark rows that follow from given camera rows, Step.model_change the model
  cost change of the step actually taken.
* tests/schur_pcg_ref.py's SchurSystem, the dense float64 restatement of the linear solve: S, b, the preconditioner and the PCG with
  its stopping rule.

GBA_STEP_MEASURED is measured, not derived (tests/test_gba_step_ref_cpu.py re-measures it and fails if a value is exceeded): the
restatement's own PCG at eta = 1e-10, followed by a plain float64 back-substitution (SchurSystem.back_substitute), evaluated in
Step.residual.  Unlike STEP_MEASURED it holds the truncation of the iteration as well as rounding, so it is kept per case and
radius; the GPU tests hold the device's step at eta = 1e-10 to 10 x the value."""
import functools
import numpy as np
import ba_step_ref as bs
import schur_pcg_ref as ref

ETA_EXACT = 1e-10
# the eta of the inexact steps the GPU tests take (the solver's default): two iterations on "259 cameras" and "chunk edges",
# recurrence residual about 0.06.  NO eta lets such a step tell the model cost change of the actual step from a formula that assumes
# S x = b: every iterate of a PCG started at zero satisfies x.(S x - b) = 0 (the residual is orthogonal to the Krylov space the
# iterate lies in), and with exactly back-substituted landmark rows that is d.(A d + g) = 0, all the shortcut
# exact_solve_model_change needs.  tests/test_gba_step_ref_cpu.py measures the agreement (1e-15 of the absolute terms) and asserts
# that off_krylov_rows, given to the step hook in place of the PCG's rows, do tell the two apart.
ETA_INEXACT = 0.1

CHUNK_EDGE_COUNTS = (513, 63, 64, 65, 255, 256, 257, 512, 513)       # observations of cameras 0..8 of "chunk edges"


def _cameras259():
    from dvslam_amd import synth
    return synth.make_ba_banded_problem(K=259, L=518, seed=259, half_span=2)


def _chunk_edges():
    """camera c keeps only its observations of the landmarks < CHUNK_EDGE_COUNTS[c]"""
    from dvslam_amd import synth
    P = synth.make_ba_problem(K=9, L=513, seed=9)
    n = np.asarray(CHUNK_EDGE_COUNTS)
    bs._trim(P, P["lm_idx"] < n[P["cam_idx"]])
    return P


def _zero_rhs():
    """cameras 0 and 1 fixed, camera 2 free and without an observation: no free camera is coupled to a landmark, b = 0"""
    from dvslam_amd import synth
    P = synth.make_ba_problem(K=3, L=40, seed=3)
    P["pose_fixed"][:] = [1, 1, 0]
    bs._trim(P, P["cam_idx"] != 2)
    return P


# name -> (builder, radii)
CASES = {
    "259 cameras": (_cameras259, (1e4, 1e-2)),
    "chunk edges": (_chunk_edges, (1e4, 1e-2)),
    "16 free of 20": (functools.partial(bs.case, "16 free of 20"), (1e4,)),
    "edges 8x150": (functools.partial(bs.case, "edges 8x150"), (1e4,)),
    "b = 0": (_zero_rhs, (1e4,)),
}
STRIDES = ("259 cameras", "chunk edges")                 # the diagonal / next-iteration tests and, with (d), the replay
TWO_SOLVERS = ("16 free of 20", "live 5x200")            # windows both device solvers take, with the same active set in both
ALL = [(n, r) for n, (_, radii) in CASES.items() for r in radii]
MEASURED_AT = ALL + [("live 5x200", 1e4)]

# Step.residual of (the restatement's PCG at ETA_EXACT, then SchurSystem.back_substitute), and the PCG iterations it ran
# (tests/test_gba_step_ref_cpu.py::test_measured_constants prints both and fails if a re-measurement exceeds the value)
GBA_STEP_MEASURED = {
    ("259 cameras", 1e4): 8.5e-11,       # measured 7.01e-11; PCG iterations at eta 0.1 / 1e-6 / 1e-10: 2 / 342 / 641
    ("259 cameras", 1e-2): 9.5e-11,      # measured 7.91e-11; 1 / 2 / 3
    ("chunk edges", 1e4): 5.4e-12,       # measured 4.44e-12; 2 / 24 / 28
    ("chunk edges", 1e-2): 7.0e-12,      # measured 5.84e-12; 1 / 2 / 3
    ("16 free of 20", 1e4): 1.5e-11,     # measured 1.22e-11; 2 / 14 / 20
    ("edges 8x150", 1e4): 2.8e-11,       # measured 2.28e-11; 2 / 11 / 17
    ("b = 0", 1e4): 6.2e-15,             # measured 5.12e-15; 0 / 0 / 0: rounding of the landmark rows alone
    ("live 5x200", 1e4): 2.8e-11,        # measured 2.27e-11; 2 / 18 / 21
}


@functools.lru_cache(maxsize=None)
def _case(name):
    return CASES[name][0]() if name in CASES else bs.case(name)


def case(name):
    """a fresh copy of the problem (a name of CASES, or of ba_step_ref.CASES)"""
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in _case(name).items()}


def case_premises(name):
    """what the case was chosen for, asserted from the problem alone"""
    P = case(name)
    K, L = int(P["K"]), int(P["L"])
    cam, lm = P["cam_idx"], P["lm_idx"]
    ncam = np.bincount(cam, minlength=K); nlm = np.bincount(lm, minlength=L)
    ca, la, slots = bs.global_active_blocks(P)
    wca, _, _ = bs.active_blocks(P)
    assert len(set(zip(cam.tolist(), lm.tolist()))) == len(cam), "a landmark at most once per camera"
    assert len(slots) >= 1
    if name == "259 cameras":
        assert (K, L, len(cam)) == (259, 518, 2578) and K > 256 and K % 4 == 3 and 6 * K + 3 * L == 3108
        assert (ncam.min(), ncam.max(), nlm.min(), nlm.max()) == (6, 10, 3, 5)
        assert P["pose_fixed"].sum() == 1 and ca[256:].all(), "free cameras on the second trip of the stride of 256"
        assert la.all() and (ca == wca).all()
    elif name == "chunk edges":
        assert (K, L) == (9, 513) and K % 4 == 1 and 6 * K + 3 * L == 1593
        assert tuple(ncam.tolist()) == CHUNK_EDGE_COUNTS
        assert P["pose_fixed"].tolist() == [1] + [0] * 8
        assert (-(-ncam // 256)).tolist() == [3, 1, 1, 1, 1, 1, 2, 2, 3], "chunks of up to 256 observations per camera"
        assert (nlm.min(), nlm.max()) == (2, 9) and la.all()
    elif name == "16 free of 20":
        bs.case_premises(name)
        assert sorted(nlm[list(bs.LDS_TRIMS)].tolist()) == [1, 4, 5, 16, 17] and (np.delete(nlm, list(bs.LDS_TRIMS)) == 20).all()
        assert (ca == wca).all(), "the same active set in both solvers"
    elif name == "live 5x200":
        bs.case_premises(name)
        assert (ca == wca).all(), "the same active set in both solvers"
    elif name == "edges 8x150":
        bs.case_premises(name)
        e = bs.EDGES["empty_cam"]
        assert ncam[e] == 0 and ca[e] and not wca[e], "the empty free camera is active here and not in the window solver"
        assert (np.delete(ca, e) == np.delete(wca, e)).all()
    elif name == "b = 0":
        assert (K, L) == (3, 40) and P["pose_fixed"].tolist() == [1, 1, 0]
        assert ncam.tolist() == [40, 40, 0] and (nlm == 2).all() and la.all()
        assert not (ca[cam]).any(), "no observation couples a free camera to a landmark"
        assert ca.tolist() == [False, False, True] and not wca.any(), "the window solver has no free camera here at all"
    else:
        raise KeyError(name)
    return P


def step(P, hpp, hll, w, g, radius, scale=None, diag=None, q=None, t=None, X=None):
    """ba_step_ref.Step with the global solver's active set, at P's point by default"""
    q, t, X = (P[k] if a is None else a for k, a in (("q", q), ("t", t), ("X", X)))
    return bs.Step(P, hpp, hll, w, g, q, t, X, radius, scale=scale, diag=diag, active=bs.global_active_blocks)


def pcg_step(P, hpp, hll, w, g, radius, eta):
    """the restatement's trial step: its PCG at eta, then the plain float64 back-substitution -> (delta [6K + 3L] in parameter
    units, x, iterations, |r| / |b| of the recurrence, ok)"""
    s = ref.SchurSystem(P, hpp, hll, w, g, radius)
    x, k, rel, ok = s.pcg(eta)
    return s.back_substitute(x), x, k, rel, ok


def off_krylov_rows(x):
    """camera rows that are no PCG iterate: coordinate j of x times 1 + cos(j) / 4.  Still a descent step, and far from satisfying
    x.(S x - b) = 0"""
    return x * (1 + 0.25 * np.cos(np.arange(len(x))))


def exact_solve_model_change(s, delta):
    """what the model cost change would be IF delta solved (H_s + D / radius) delta = -g_s: then delta^T H_s delta =
    -delta.g_s - delta^T (D / radius) delta, and -(delta.g_s + delta^T H_s delta / 2) = (delta^T (D / radius) delta - delta.g_s) / 2.
    A kernel that took this shortcut would be right for a direct solve and wrong for an inexact one."""
    d = s.scaled(delta)[s.idx]
    return (d @ (s.diag[s.idx] / bs.LD(s.radius) * d) - d @ s.gs[s.idx]) / 2
