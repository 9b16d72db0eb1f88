"""Pose-graph optimisation without a GPU: the dvs_pgo_* symbols declared and exported (both ways), the header as C, argument errors without
a device, the C++ adapter under g++ -Wall -Werror, and the float64 restatement (tests/pose_graph_ref.py) against independent second
statements: residuals against scipy.spatial.transform.Rotation, Jacobians against central differences, the ref's Levenberg-Marquardt
against scipy.optimize.least_squares on every graph.

This file also MEASURES the constants the GPU tests use and asserts they do not exceed what pose_graph_ref.py carries:
  LIN_MEASURED         float64 linearize() against the same formulas in numpy.longdouble (64-bit mantissa on x86-64), in the
                       distance of pose_graph_ref.lin_distance, over every graph;
  EXACT_POSE_MEASURED  what the ref's LM leaves against the planted poses on `exact24`;
  PCG_X_MEASURED       the ref's float64 PCG at eta = 1e-12 against numpy.linalg.solve on the systems the GPU hook test solves;
  SCIPY_COST           scipy's final cost per graph (recorded so that the GPU tests do not run scipy)."""
import ctypes as C
import functools
import os
import re
import subprocess
import numpy as np
import pytest

import pose_graph_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "dynamic-visual-slam_amd", "lib")
SYMBOLS = ["dvs_pgo_default_params", "dvs_pgo_check_graph", "dvs_pgo_create", "dvs_pgo_destroy", "dvs_pgo_synchronize", "dvs_pgo_set_nodes",
           "dvs_pgo_set_edges", "dvs_pgo_evaluate", "dvs_pgo_solve", "dvs_pgo_get_nodes", "dvs_pgo_get_trace", "dvs_pgo_correct_points",
           "dvs_pgo_correct_points_device"]
HOOKS = ["dvs_test_pgo_apply", "dvs_test_pgo_pcg", "dvs_test_pgo_trial_step"]


def _exports(name):
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(LIBDIR, name)], capture_output=True, text=True, check=True).stdout
    return set(line.split()[-1] for line in out.splitlines() if line.strip())


def test_symbols_declared_and_exported_both_ways(hiplib, hooks):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dvslam_hip.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(dvs_pgo_[a-z0-9_]+)\s*\(", hdr)))
    product, test = _exports("libdvslam_hip.so"), _exports("libdvslam_hip_test.so")
    assert declared == sorted(SYMBOLS)
    assert sorted(n for n in product if n.startswith("dvs_pgo_")) == sorted(SYMBOLS)
    assert set(SYMBOLS) <= test
    thdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dvslam_hip_test_pgo.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(dvs_test_[a-z0-9_]+)\s*\(", thdr))) == HOOKS
    assert not [n for n in HOOKS if n in product] and set(HOOKS) <= test
    assert '#include "dvslam_hip_test_pgo.h"' in open(os.path.join(ROOT, "include", "dvslam_hip_test.h")).read()


def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "pgo.c"
    src.write_text('#include "dvslam_hip_test.h"\nint main(void) { dvs_pgo* h = 0; dvs_pgo_params p; dvs_pgo_summary s; s.termination = 0; '
                   'return dvs_pgo_default_params(&p) + s.termination + (h != 0); }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "pgo.o")])


def test_null_handles_and_defaults(hiplib):
    from dvslam_amd._lib import PgoParams, PgoSummary
    L = hiplib
    p = PgoParams(max_iterations=1, eta=0.9)
    assert L.dvs_pgo_default_params(None) == -6 and L.dvs_pgo_default_params(C.byref(p)) == 0
    d = pr.DEFAULTS
    assert [p.max_iterations, p.max_pcg_iterations, p.function_tolerance, p.gradient_tolerance, p.parameter_tolerance, p.eta] == \
        [d[k] for k in ("max_iterations", "max_pcg_iterations", "function_tolerance", "gradient_tolerance", "parameter_tolerance", "eta")]
    assert C.sizeof(PgoParams) == 40 and C.sizeof(PgoSummary) == 32
    n, s = C.c_int32(), PgoSummary()
    assert L.dvs_pgo_create(0, None) == -6
    assert L.dvs_pgo_set_nodes(None, 0, None, None, None) == -6 and L.dvs_pgo_set_edges(None, 0, None, None, None, None, None, None) == -6
    assert L.dvs_pgo_evaluate(None, None, None, None, None, None) == -6 and L.dvs_pgo_solve(None, C.byref(p), C.byref(s)) == -6
    assert L.dvs_pgo_get_nodes(None, None, None) == -6 and L.dvs_pgo_get_trace(None, None, 0, C.byref(n)) == -6
    assert L.dvs_pgo_correct_points(None, 0, None, None) == -6 and L.dvs_pgo_correct_points_device(None, 0, None, None) == -6
    assert L.dvs_pgo_synchronize(None) == -6
    L.dvs_pgo_destroy(None)


def _check(L, g, **over):
    from dvslam_amd._lib import ptr
    a = dict(N=g.N, R=g.R, t=g.t, fixed=g.fixed, E=g.E, i=g.ei, j=g.ej, rvec=g.rvec, tvec=g.tvec, w_rot=g.w_rot, w_trans=g.w_trans)
    a.update(over)
    keep = {k: (np.ascontiguousarray(v) if isinstance(v, np.ndarray) else v) for k, v in a.items()}
    f = lambda k: ptr(keep[k]) if keep[k] is not None else None
    return L.dvs_pgo_check_graph(keep["N"], f("R"), f("t"), f("fixed"), keep["E"], f("i"), f("j"), f("rvec"), f("tvec"), f("w_rot"), f("w_trans"))


def test_argument_errors_without_a_device(hiplib):
    """dvs_pgo_check_graph runs the very checks of dvs_pgo_set_nodes / dvs_pgo_set_edges (one pair of functions in csrc/pose_graph.hip)"""
    g = pr.graph("ring24")
    L = hiplib
    assert _check(L, g) == 0

    def changed(arr, idx, val):
        out = arr.copy(); out[idx] = val
        return out
    assert _check(L, g, fixed=np.zeros(g.N, np.uint8)) == -6                          # no fixed node
    assert _check(L, g, j=changed(g.ej, 3, g.ei[3])) == -6                            # i == j
    assert _check(L, g, i=changed(g.ei, 0, -1)) == -6 and _check(L, g, j=changed(g.ej, 5, g.N)) == -6
    assert _check(L, g, w_rot=changed(g.w_rot, 2, 0.0)) == -6 and _check(L, g, w_trans=changed(g.w_trans, 2, -1.0)) == -6
    assert _check(L, g, w_rot=changed(g.w_rot, 2, np.inf)) == -6 and _check(L, g, w_trans=changed(g.w_trans, 2, np.nan)) == -6
    assert _check(L, g, R=changed(g.R, (4, 1, 1), np.nan)) == -6 and _check(L, g, t=changed(g.t, (4, 1), np.inf)) == -6
    assert _check(L, g, rvec=changed(g.rvec, (7, 0), np.nan)) == -6 and _check(L, g, tvec=changed(g.tvec, (7, 2), -np.inf)) == -6
    assert _check(L, g, N=0) == -6 and _check(L, g, N=(1 << 20) + 1) == -6 and _check(L, g, E=0) == -6 and _check(L, g, E=(1 << 22) + 1) == -6
    assert _check(L, g, R=None) == -6 and _check(L, g, i=None) == -6 and _check(L, g, w_trans=None) == -6
    assert _check(L, g, fixed=np.zeros(g.N, np.uint8)) == -6 and b"no fixed node" in L.dvs_last_error()


def _build_adapter(tmpdir):
    exe = os.path.join(str(tmpdir), "pose_graph_adapter")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "pose_graph_adapter.cpp"), "-o", exe, "-L" + LIBDIR, "-ldvslam_hip",
                           "-Wl,-rpath," + LIBDIR, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_adapter_compiles_and_refuses_without_gpu(tmp_path, hiplib):
    from dvslam_amd import device_count
    code = subprocess.call([_build_adapter(tmp_path)], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    assert code == (2 if device_count() > 0 else 3)       # with a GPU and no arguments: the usage exit


# ------------------------------------------------------------------------------------------------ the restatement on its own
def test_residuals_equal_a_scipy_rotation_statement():
    """r = [w_rot rotvec(Z^-1 T_i^-1 T_j) ; w_trans trans(Z^-1 T_i^-1 T_j)] composed from 4 x 4 matrices, the log by scipy"""
    from scipy.spatial.transform import Rotation

    def T(R, t):
        M = np.eye(4); M[:3, :3] = R; M[:3, 3] = t
        return M
    for name in pr.ALL_GRAPHS:
        g = pr.graph(name)
        res = pr.linearize(g)[1]
        for e in range(g.E):
            i, j = g.ei[e], g.ej[e]
            Z = T(Rotation.from_rotvec(g.rvec[e]).as_matrix(), g.tvec[e])
            Err = np.linalg.inv(Z) @ np.linalg.inv(T(g.R[i], g.t[i])) @ T(g.R[j], g.t[j])
            want = np.concatenate([g.w_rot[e] * Rotation.from_matrix(Err[:3, :3]).as_rotvec(), g.w_trans[e] * Err[:3, 3]])
            assert np.abs(res[e] - want).max() <= 1e-9 * max(1.0, np.abs(want).max()), (name, e)


def _retract(R, t, d):
    return R @ pr.rodrigues(d[:3]), t + R @ d[3:]


def test_jacobians_equal_central_differences():
    h = 1e-6
    for name in ("ring24",) + pr.EDGE_CASES:
        g = pr.graph(name)
        _, _, A, B, _ = pr.linearize(g)
        for e in range(g.E):
            i, j = int(g.ei[e]), int(g.ej[e])
            Rz = pr.rodrigues(g.rvec[e])
            for blk, side in ((A[e], 0), (B[e], 1)):
                if g.fixed[(i, j)[side]]:
                    assert not blk.any()
                    continue
                num = np.zeros((6, 6))
                for c in range(6):
                    d = np.zeros(6); d[c] = h
                    out = []
                    for sgn in (1, -1):
                        Ri, ti, Rj, tj = g.R[i], g.t[i], g.R[j], g.t[j]
                        if side == 0:
                            Ri, ti = _retract(Ri, ti, sgn * d)
                        else:
                            Rj, tj = _retract(Rj, tj, sgn * d)
                        out.append(pr.edge_terms(Ri, ti, Rj, tj, Rz, g.tvec[e], g.w_rot[e], g.w_trans[e])[0])
                    num[:, c] = (out[0] - out[1]) / (2 * h)
                # central differences: truncation h^2 |r'''| and rounding eps |r| / h, both scaled by the block's size
                assert np.abs(blk - num).max() <= 1e-6 * max(1.0, np.abs(blk).max()), (name, e, side)


def test_scipy_jacobian_equals_central_differences():
    g = pr.graph("two_fixed")
    s = pr.scipy_solve(g)
    x = s["x0"] + 0.01
    J = s["jac"](x)
    num = np.zeros_like(J)
    for c in range(len(x)):
        d = np.zeros(len(x)); d[c] = 1e-6
        num[:, c] = (s["fun"](x + d) - s["fun"](x - d)) / 2e-6
    assert np.abs(J - num).max() <= 1e-6 * np.abs(J).max()


@functools.lru_cache(maxsize=None)
def _ref_solve(name):
    return pr.solve(pr.graph(name), pr.TIGHT)


@pytest.mark.parametrize("name", pr.ALL_GRAPHS)
def test_ref_lm_equals_scipy_least_squares(name):
    g = pr.graph(name)
    s = _ref_solve(name)
    sc = pr.scipy_solve(g)["cost"]
    print(f"{name}: ref {s['final_cost']!r} scipy {sc!r} steps {s['num_successful_steps']} pcg {s['pcg_iterations']}")
    assert s["termination"] == 0 and s["final_cost"] <= s["initial_cost"]
    assert abs(s["final_cost"] - sc) <= 1e-6 * sc + pr.ZERO_COST
    assert abs(pr.SCIPY_COST[name] - sc) <= 1e-9 * sc + pr.ZERO_COST          # the recorded value the GPU tests use
    assert sum(r[6] for r in s["trace"]) == s["pcg_iterations"]
    if name == "isolated":
        assert (s["R"][6] == pr.R_from_quat(pr.quat_from_R(g.R[6]))).all() and (s["t"][6] == g.t[6]).all()
    if name == "two_fixed":
        assert (s["t"][[0, 3]] == g.t[[0, 3]]).all()


def test_measured_constants():
    assert np.finfo(np.longdouble).nmant >= 63, "numpy.longdouble has no wider mantissa than float64 here: nothing is measured"
    lin = 0.0
    for name in pr.ALL_GRAPHS:
        g = pr.graph(name)
        a, b = pr.linearize(g), pr.linearize(g, dtype=np.longdouble)
        lin = max(lin, pr.lin_distance(g, a, b))
    g = pr.graph("exact24")
    s = _ref_solve("exact24")
    exact = max(np.abs(s["R"] - g.planted[0]).max(), np.abs(s["t"] - g.planted[1]).max())
    pcgx = 0.0
    for name, radius in pr.PCG_CASES:
        g = pr.graph(name)
        _, _, A, B, grad = pr.linearize(g)
        J = pr.dense_jacobian(g, A, B); H = J.T @ J
        D = pr.lm_diagonal(H, g.fixed)
        x, it, rn, gn = pr.pcg(H, D, radius, grad, g.fixed, 1e-12, pr.PCG_TIGHT_MAX_IT)
        free = np.repeat(g.fixed == 0, 6)
        want = np.zeros_like(x)
        want[free] = np.linalg.solve((H + np.diag(D / radius))[np.ix_(free, free)], -grad[free])
        pcgx = max(pcgx, float(np.linalg.norm(x - want) / np.linalg.norm(want)))
        print(f"pcg {name} radius {radius}: {it} iterations, |r|/|g| {rn / gn:.2e}")
        x1, it1, rn1, gn1 = pr.pcg(H, D, radius, grad, g.fixed, 0.1, 1000)
        assert 1 <= it1 < 1000 and rn1 <= 0.1 * gn1
    print(f"LIN_MEASURED {lin:.3e}  EXACT_POSE_MEASURED {exact:.3e}  PCG_X_MEASURED {pcgx:.3e}")
    assert 0 < lin <= pr.LIN_MEASURED
    assert 0 < exact <= pr.EXACT_POSE_MEASURED
    assert 0 < pcgx <= pr.PCG_X_MEASURED


def test_correct_points_restatement():
    g = pr.graph("ring24")
    s = _ref_solve("ring24")
    rng = np.random.default_rng(4)
    xyz = rng.uniform(-6, 6, (40, 3)).astype(np.float32)
    anchor = rng.integers(0, g.N, 40).astype(np.int32); anchor[3] = -1; anchor[9] = g.N
    out = pr.correct_points(xyz, anchor, g.R, g.t, s["R"], s["t"])
    assert (out[[3, 9]] == xyz[[3, 9]]).all()
    for k in (0, 1, 2, 4):
        a = anchor[k]
        want = s["R"][a] @ (g.R[a].T @ (xyz[k].astype(np.float64) - g.t[a])) + s["t"][a]
        assert np.abs(out[k] - want).max() <= 1e-5
    same = pr.correct_points(xyz, anchor, g.R, g.t, g.R, g.t)                 # nothing moved: the points come back to rounding
    assert np.abs(same - xyz).max() <= 2e-6
