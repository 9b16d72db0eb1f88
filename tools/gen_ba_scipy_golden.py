#!/usr/bin/env python3
"""Independent statement of the sliding-window BA optimum (the LM loop of dvs_ba_solve* was only ever
checked against its own transcription in oracle/ba_oracle.cpp).

Solves the synthetic windows 3x60, 5x200, 10x2000 and 24x300 (dvslam_amd.synth.make_ba_problem, the generator bench.py and the tests
use) and the banded 80x400 problem (make_ba_banded_problem) with scipy.optimize.least_squares(method="trf") to convergence and
stores the optimum under tests/golden/ba_scipy_*.npz.  Nothing here shares code with csrc/ba.hip or oracle/ba_oracle.cpp:

* residual model written from bundle_adjustment.hpp:531-565 in numpy (rotation matrices, not the quaternion sandwich);
* poses parameterised MINIMALLY as q = q_init (x) exp(omega), omega in R^3 (not Ceres' ambient quaternion + manifold);
* Ceres applies HuberLoss(1.345) to the squared NORM s = |r|^2 of each 2-vector residual block (bundle_adjustment.hpp:818):
  rho(s) = s (s <= a^2), 2 a sqrt(s) - a^2 otherwise, cost 0.5 * sum rho.  scipy's loss="huber" acts per SCALAR residual, which
  is a different objective for 2-vector blocks (and feeding it the block norm |r| as one scalar leaves a rank-1 Gauss-Newton
  model that stalls: tried, stopped at 3x the optimum's cost).  So the loss is folded into the residual instead, exactly:
  g = r * sqrt(rho(s)) / |r|, a 2-vector with |g|^2 = rho(s), handed to a PLAIN least-squares solve (loss="linear"), whose
  objective 0.5 * sum |g|^2 IS Ceres' robustified cost;
* a different trust-region method (reflective trf with lsmr steps, no Schur complement, no loss corrector) from a different
  code base, with finite-difference Jacobians.

The optimum COST is parameterisation- and method-independent; poses agree only up to the gauge the problem leaves free
(first pose fixed => global scale is a null direction of a monocular window), which is how tests/test_gpu_ba.py compares them."""
import os
import sys
import time

import numpy as np
from scipy.optimize import least_squares
from scipy.sparse import lil_matrix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dynamic-visual-slam_amd"))
from dvslam_amd import synth  # noqa: E402

HUBER = 1.345
# 3x60 without the 2 % outlier observations: with only three views per landmark and a linear-growth loss, a landmark that carries an
# outlier has several local minima (fit the outlier or fit the other two views), and the two solvers settle in different ones
# (measured: 804.2 vs 1539.1 — the LM loop found the LOWER one); with >= 5 views the outliers cannot win and the basins coincide.
CASES = [("3x60", dict(K=3, L=60, seed=9, outlier_frac=0.0)), ("5x200", dict(K=5, L=200, seed=7)), ("10x2000", dict(K=10, L=2000, seed=42)),
         # a window beyond 16 free keyframes with partial co-visibility (dvs_ba_set_device_window; tests/test_gpu_ba_window.py)
         ("24x300", dict(K=24, L=300, seed=24, visibility=0.6)),
         # a banded problem with more cameras than any window (dvs_ba_solve_global; tests/test_gpu_ba_global.py).  The third entry: the
         # generator when it is not make_ba_problem, and exact=True for trf's dense SVD steps (tr_solver="exact") on a dense Jacobian:
         # with lsmr steps this chain of 80 cameras creeps along the scale gauge's valley — 54689.68, 54689.55, 54689.48, 54689.42,
         # 54689.39 after rounds of 300 evaluations — while the exact steps reach 54688.0787254513 in 61 evaluations and stay there.
         ("80x400_banded", dict(K=80, L=400, seed=80, half_span=4), dict(generator="make_ba_banded_problem", exact=True))]


def rot_from_quat(q):
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def exp_so3(w):
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / (th * th) * (K @ K)


def quat_from_rot(R):
    """Shepperd; sign chosen positive w (the comparison is sign-agnostic)"""
    tr = np.trace(R)
    if tr > 0:
        s = np.sqrt(tr + 1.0) * 2
        q = np.array([0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s])
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0) * 2
        q = np.zeros(4)
        q[0] = (R[k, j] - R[j, k]) / s
        q[1 + i] = 0.25 * s
        q[1 + j] = (R[j, i] + R[i, j]) / s
        q[1 + k] = (R[k, i] + R[i, k]) / s
    return q / np.linalg.norm(q)


class Window:
    def __init__(self, P):
        self.P = P
        self.K, self.L = P["K"], P["L"]
        self.R0 = [rot_from_quat(P["q"][k]) for k in range(self.K)]
        self.free = [k for k in range(self.K) if not P["pose_fixed"][k]]
        self.slot = {k: i for i, k in enumerate(self.free)}
        self.nf = len(self.free)

    def unpack(self, x):
        Rs = list(self.R0); ts = [self.P["t"][k].copy() for k in range(self.K)]
        for k in self.free:
            o = 6 * self.slot[k]
            Rs[k] = self.R0[k] @ exp_so3(x[o:o + 3])
            ts[k] = x[o + 3:o + 6]
        X = x[6 * self.nf:].reshape(self.L, 3)
        return Rs, ts, X

    def x0(self):
        x = np.zeros(6 * self.nf + 3 * self.L)
        for k in self.free:
            x[6 * self.slot[k] + 3:6 * self.slot[k] + 6] = self.P["t"][k]
        x[6 * self.nf:] = self.P["X"].reshape(-1)
        return x

    def block_residuals(self, x):
        P = self.P
        Rs, ts, X = self.unpack(x)
        Rm = np.stack(Rs)[P["cam_idx"]]; tm = np.stack(ts)[P["cam_idx"]]
        pc = np.einsum("nij,nj->ni", Rm, X[P["lm_idx"]]) + tm
        ok = ~(pc[:, 2] <= 0.1)                                  # bundle_adjustment.hpp:545-550
        z = np.where(ok, pc[:, 2], 1.0)
        r = np.stack([P["fx"] * pc[:, 0] / z + P["cx"] - P["uv"][:, 0], P["fy"] * pc[:, 1] / z + P["cy"] - P["uv"][:, 1]], axis=1) / P["sigma"]
        return r * ok[:, None]

    def fun(self, x):
        r = self.block_residuals(x)
        n = np.linalg.norm(r, axis=1)
        big = n > HUBER
        scale = np.ones_like(n)
        scale[big] = np.sqrt(2 * HUBER * n[big] - HUBER ** 2) / n[big]
        return (r * scale[:, None]).reshape(-1)

    def cost(self, x):
        s = (self.block_residuals(x) ** 2).sum(axis=1)
        rho = np.where(s <= HUBER ** 2, s, 2 * HUBER * np.sqrt(s) - HUBER ** 2)
        return 0.5 * rho.sum()

    def sparsity(self):
        n = len(self.P["cam_idx"])
        S = lil_matrix((2 * n, 6 * self.nf + 3 * self.L), dtype=np.int8)
        for i in range(n):
            k = int(self.P["cam_idx"][i]); l = int(self.P["lm_idx"][i])
            for row in (2 * i, 2 * i + 1):
                if k in self.slot:
                    S[row, 6 * self.slot[k]:6 * self.slot[k] + 6] = 1
                S[row, 6 * self.nf + 3 * l:6 * self.nf + 3 * l + 3] = 1
        return S.tocsr()


def solve(P, verbose=0, exact=False):
    W = Window(P)
    x = W.x0()
    c0 = W.cost(x)
    best = None
    if exact:
        from scipy.optimize._numdiff import approx_derivative
        sparsity = W.sparsity()
        how = dict(jac=lambda x: approx_derivative(W.fun, x, method="3-point", sparsity=sparsity).toarray(), tr_solver="exact", max_nfev=100)
    else:
        how = dict(jac="3-point", jac_sparsity=W.sparsity(), max_nfev=300)
    for rnd in range(6):        # restart until the cost no longer moves: scipy's own stopping rules are not Ceres'
        sol = least_squares(W.fun, x, method="trf", loss="linear", xtol=1e-15, ftol=1e-15, gtol=1e-15, x_scale="jac", verbose=verbose, **how)
        x = sol.x
        c = W.cost(x)
        if best is not None and abs(best - c) <= 1e-10 * c:
            best = min(best, c)
            break
        best = c if best is None else min(best, c)
    assert abs(sol.cost - W.cost(x)) <= 1e-9 * W.cost(x), "scipy's robust cost must equal 0.5 * sum rho_huber(|r|^2)"
    Rs, ts, X = W.unpack(x)
    q = np.stack([quat_from_rot(R) for R in Rs]); t = np.stack(ts)
    return c0, best, q, t, X.copy()


def main():
    import json
    out_dir = os.path.join(ROOT, "tests", "golden")
    only = sys.argv[1:]
    for name, kw, *more in CASES:
        if only and name not in only:
            continue
        opts = more[0] if more else {}
        generator = opts.get("generator", "make_ba_problem")
        P = getattr(synth, generator)(**kw)
        t0 = time.time()
        c0, c, q, t, X = solve(P, exact=opts.get("exact", False))
        print(f"{name}: initial cost {c0:.9g} -> optimum {c:.12g}  ({time.time() - t0:.1f} s)", flush=True)
        np.savez_compressed(os.path.join(out_dir, f"ba_scipy_{name}.npz"), make_ba_problem_kwargs=json.dumps(kw), initial_cost=c0,
                            optimum_cost=c, q=q, t=t, X=X.astype(np.float64), **({"generator": generator} if more else {}))


if __name__ == "__main__":
    main()
