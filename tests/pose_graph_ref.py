"""The pose-graph rule of include/dvslam_hip.h ("Pose-graph optimisation", dvs_pgo_*) restated sequentially in float64 numpy with dense
linear algebra, the test graphs, and the constants the GPU tests use.  Nothing here is the kernel: sums run one term after the other,
the linear algebra is dense, and every function takes the number type from its inputs so that tests/test_pose_graph_cpu.py can run the
same formulas in numpy.longdouble and MEASURE how far float64 is from them.

  LIN_MEASURED         the largest distance, relative to the largest magnitude of each quantity (residuals, Jacobian blocks, gradient,
                       cost), between linearize() in float64 and in longdouble over every test graph.
  EXACT_POSE_MEASURED  the largest |delta (R, t)| the ref's own LM leaves against the planted poses on `exact24`.
  PCG_X_MEASURED       |x - numpy.linalg.solve| / |solve| of the ref's float64 PCG at eta = 1e-12 on the hook's systems.
The constants below were taken from a run of tests/test_pose_graph_cpu.py, which asserts that the measurements do not exceed them."""
import functools
import math
import numpy as np

LIN_MEASURED = 6.0e-16          # measured 5.67e-16
EXACT_POSE_MEASURED = 2.0e-14   # measured 1.91e-14
PCG_X_MEASURED = 8.0e-11        # measured 7.55e-11
# the step tests' constants (tests/test_pose_graph_steps_cpu.py measures them and asserts they are not exceeded):
#   TRIAL_MEASURED     trial_step() in float64 against longdouble at the same poses and step, in trial_distance(), over every replayed step
#   PCG_STEP_MEASURED  the float64 PCG against pcg_k() in longdouble on the same system at the same iteration, |x - x_ld| / |x_ld|, per graph
TRIAL_MEASURED = 9.0e-16        # measured 8.55e-16
PCG_STEP_MEASURED = {"ring24_far": 2.0e-14, "ring24_far2": 3.0e-15, "chain515": 2.0e-15, "hub300": 3.0e-14}   # measured 1.72e-14, 2.51e-15, 1.92e-15, 2.79e-14

# costs below this are zero to rounding (residuals of w eps |t|, about 1e-13, squared): the relative brackets add it as an absolute floor
ZERO_COST = 1e-20
# scipy.optimize.least_squares' final cost per graph (scipy_solve below); tests/test_pose_graph_cpu.py checks each against a fresh run
SCIPY_COST = {"ring24": 5.519908971873887, "hub300": 205.07267987146153, "exact24": 4.0049775814151506e-26, "two_nodes": 1.8298569980513458e-28,
              "isolated": 2.3588847068375154, "duplicate": 2.536966191256407, "zero_rot": 36521.454283833395, "tiny_rot": 4.076360034101816,
              "big_rot": 53914.384141335024, "two_fixed": 5.549511487739648}
# the systems the linear-solve hook test solves: (graph, radius), at the graph's initial linearisation
PCG_CASES = (("ring24", 1e4), ("ring24", 1.0), ("hub300", 1e4))
PCG_TIGHT_MAX_IT = 2000
# the same on the graph whose 515 nodes and 517 edges take the single-workgroup loops (512 threads) through a second trip.  The long chain
# is worse conditioned at radius 1e4 (1350 iterations): its systems have PCG_X_MEASURED's of their own, measured in the same way
SECOND_TRIP_GRAPHS = ("chain515", "chain515_fixed")
SECOND_TRIP_PCG_CASES = (("chain515", 1e4), ("chain515", 1.0))
PCG_X_MEASURED_SECOND_TRIP = {("chain515", 1e4): 1.2e-9, ("chain515", 1.0): 4.0e-12}   # measured 1.11e-09, 3.54e-12


def pcg_x_measured(name, radius):
    return PCG_X_MEASURED_SECOND_TRIP.get((name, radius), PCG_X_MEASURED)


DEFAULTS = dict(max_iterations=50, function_tolerance=1e-6, gradient_tolerance=1e-10, parameter_tolerance=1e-8, eta=0.1, max_pcg_iterations=0)
# what the solve tests pass: the function tolerance of the default would stop within 1e-6 of the minimum, which IS the tests' bracket
TIGHT = dict(DEFAULTS, max_iterations=100, function_tolerance=1e-14, parameter_tolerance=1e-14)


# ---------------------------------------------------------------------------------------------------------------- SO(3)
def hat(w):
    z = w[0] * 0
    return np.array([[z, -w[2], w[1]], [w[2], z, -w[0]], [-w[1], w[0], z]], dtype=w.dtype)


def rodrigues(rvec):
    """R of a rotation vector: cos I + (1 - cos) k k^T + sin [k]x with k = rvec / |rvec|; the identity for the zero vector"""
    rvec = np.asarray(rvec)
    th = np.sqrt(rvec[0] * rvec[0] + rvec[1] * rvec[1] + rvec[2] * rvec[2])
    if th == 0:
        return np.eye(3, dtype=rvec.dtype)
    k = rvec / th
    c, s = np.cos(th), np.sin(th)
    return c * np.eye(3, dtype=rvec.dtype) + (1 - c) * np.outer(k, k) + s * hat(k)


def so3_log(Q):
    """the rule's Log: (omega, theta)"""
    v = np.array([Q[2, 1] - Q[1, 2], Q[0, 2] - Q[2, 0], Q[1, 0] - Q[0, 1]], dtype=Q.dtype) / 2
    s = np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    c = (Q[0, 0] + Q[1, 1] + Q[2, 2] - 1) / 2
    th = np.arctan2(s, c)
    return (v * (th / s) if s > 1e-12 else v), th


def jr_inv(w, th):
    """inverse right Jacobian of SO(3): I + [w]x / 2 + c [w]x^2, c = 1/th^2 - (1 + cos th) / (2 th sin th); its series below 1e-2"""
    if th < 1e-2:
        t2 = th * th
        c = 1 / w.dtype.type(12) + t2 / 720 + t2 * t2 / 30240
    else:
        c = 1 / (th * th) - (1 + np.cos(th)) / (2 * th * np.sin(th))
    W = hat(w)
    return np.eye(3, dtype=w.dtype) + W / 2 + c * (W @ W)


def quat_from_R(R):
    """(w, x, y, z), w >= 0 ... by the largest of the four (Shepperd), normalised"""
    R = np.asarray(R, dtype=np.float64)
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    if tr > 0:
        s = math.sqrt(tr + 1.0) * 2
        q = [0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s]
    elif R[0, 0] > R[1, 1] and R[0, 0] > R[2, 2]:
        s = math.sqrt(1.0 + R[0, 0] - R[1, 1] - R[2, 2]) * 2
        q = [(R[2, 1] - R[1, 2]) / s, 0.25 * s, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s]
    elif R[1, 1] > R[2, 2]:
        s = math.sqrt(1.0 + R[1, 1] - R[0, 0] - R[2, 2]) * 2
        q = [(R[0, 2] - R[2, 0]) / s, (R[0, 1] + R[1, 0]) / s, 0.25 * s, (R[1, 2] + R[2, 1]) / s]
    else:
        s = math.sqrt(1.0 + R[2, 2] - R[0, 0] - R[1, 1]) * 2
        q = [(R[1, 0] - R[0, 1]) / s, (R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, 0.25 * s]
    q = np.array(q)
    return q / math.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])


def R_from_quat(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]], dtype=np.asarray(q).dtype)


def quat_mul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])


def quat_exp(w):
    th = math.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    if th == 0:
        return np.array([1.0, 0, 0, 0])
    s = math.sin(th / 2) / th
    return np.array([math.cos(th / 2), s * w[0], s * w[1], s * w[2]])


# ---------------------------------------------------------------------------------------------------------------- the rule
class Graph:
    """nodes R [N][3][3], t [N][3], fixed [N]; edges i, j, rvec, tvec, w_rot, w_trans; planted poses where the graph has them"""

    def __init__(self, R, t, fixed, ei, ej, rvec, tvec, w_rot, w_trans, planted=None):
        self.R = np.ascontiguousarray(R, dtype=np.float64); self.t = np.ascontiguousarray(t, dtype=np.float64)
        self.fixed = np.ascontiguousarray(fixed, dtype=np.uint8)
        self.ei = np.ascontiguousarray(ei, dtype=np.int32); self.ej = np.ascontiguousarray(ej, dtype=np.int32)
        self.rvec = np.ascontiguousarray(rvec, dtype=np.float64).reshape(-1, 3); self.tvec = np.ascontiguousarray(tvec, dtype=np.float64).reshape(-1, 3)
        self.w_rot = np.ascontiguousarray(w_rot, dtype=np.float64); self.w_trans = np.ascontiguousarray(w_trans, dtype=np.float64)
        self.planted = planted
        self.N, self.E = len(self.R), len(self.ei)


def edge_terms(Ri, ti, Rj, tj, Rz, tz, wr, wt, fixed_i=False, fixed_j=False):
    """residual (6) and the two 6 x 6 blocks A = d r / d delta_i, B = d r / d delta_j at delta = 0"""
    M = Ri.T @ Rj
    Q = Rz.T @ M
    w, th = so3_log(Q)
    p = Ri.T @ (tj - ti)
    r = np.concatenate([wr * w, wt * (Rz.T @ (p - tz))])
    Ji = jr_inv(w, th)
    A = np.zeros((6, 6), dtype=Ri.dtype); B = np.zeros((6, 6), dtype=Ri.dtype)
    if not fixed_i:
        A[:3, :3] = -wr * (Ji @ M.T)
        A[3:, :3] = wt * (Rz.T @ hat(p))
        A[3:, 3:] = -wt * Rz.T
    if not fixed_j:
        B[:3, :3] = wr * Ji
        B[3:, 3:] = wt * Q
    return r, A, B


def linearize(g, R=None, t=None, dtype=np.float64):
    """(cost, res [E][6], A [E][6][6], B [E][6][6], grad [6N]) — sums in ascending edge index"""
    R = (g.R if R is None else R).astype(dtype); t = (g.t if t is None else t).astype(dtype)
    res = np.zeros((g.E, 6), dtype); A = np.zeros((g.E, 6, 6), dtype); B = np.zeros((g.E, 6, 6), dtype)
    grad = np.zeros(6 * g.N, dtype)
    cost = dtype(0)
    for e in range(g.E):
        i, j = int(g.ei[e]), int(g.ej[e])
        Rz = rodrigues(g.rvec[e].astype(dtype))
        res[e], A[e], B[e] = edge_terms(R[i], t[i], R[j], t[j], Rz, g.tvec[e].astype(dtype), dtype(g.w_rot[e]), dtype(g.w_trans[e]),
                                        bool(g.fixed[i]), bool(g.fixed[j]))
        grad[6 * i:6 * i + 6] += A[e].T @ res[e]
        grad[6 * j:6 * j + 6] += B[e].T @ res[e]
        cost += res[e] @ res[e]
    return cost / 2, res, A, B, grad


def lin_distance(g, got, want):
    """the distance LIN_MEASURED is stated in: per quantity of linearize()'s tuple, max |got - want| over the quantity's scale, the largest
    of them.  The scale is the quantity's largest magnitude, but not less than the size of the terms that cancel in it — w (1 + |t|) for a
    residual (a noise-free edge leaves rounding only), that times the largest Jacobian entry for the gradient, its square for the cost."""
    want = [np.asarray(x, np.longdouble) for x in want]
    got = [np.asarray(x, np.longdouble) for x in got]
    s_r = max(float(np.abs(want[1]).max()), float(max(g.w_rot.max(), g.w_trans.max()) * max(1.0, np.abs(g.t).max())))
    s_j = max(float(np.abs(want[2]).max()), float(np.abs(want[3]).max()))
    scale = [max(float(want[0]), s_r * s_r), s_r, s_j, s_j, max(float(np.abs(want[4]).max()), s_r * s_j)]
    return max(float(np.abs(a - b).max()) / sc for a, b, sc in zip(got, want, scale))


def residual_vector(g, R, t):
    out = np.zeros((g.E, 6))
    for e in range(g.E):
        i, j = int(g.ei[e]), int(g.ej[e])
        out[e] = edge_terms(R[i], t[i], R[j], t[j], rodrigues(g.rvec[e]), g.tvec[e], g.w_rot[e], g.w_trans[e])[0]
    return out.ravel()


def dense_jacobian(g, A, B):
    J = np.zeros((6 * g.E, 6 * g.N), dtype=A.dtype)
    for e in range(g.E):
        i, j = int(g.ei[e]), int(g.ej[e])
        J[6 * e:6 * e + 6, 6 * i:6 * i + 6] += A[e]
        J[6 * e:6 * e + 6, 6 * j:6 * j + 6] += B[e]
    return J


def lm_diagonal(H, fixed):
    """clamp(diag(H), 1e-6, 1e32); zero on fixed nodes, whose rows are not part of the system"""
    D = np.clip(np.diag(H), 1e-6, 1e32)
    return D * np.repeat(1 - np.asarray(fixed, dtype=np.float64), 6)


def pcg(H, D, radius, gvec, fixed, eta, max_it, hist=None):
    """(x, iterations, |r|, |g|): block-Jacobi preconditioned CG on (H + D / radius) x = -g, zero start, over the free rows.  hist, a list,
    receives |r| / (eta |g|) of the start and of every iteration: how far each stopping test was from its threshold."""
    n = len(gvec)
    free = np.repeat(np.asarray(fixed) == 0, 6)
    Am = H + np.diag(D / radius)
    Minv = np.zeros((n, n))
    for k in range(0, n, 6):
        if free[k]:
            Minv[k:k + 6, k:k + 6] = np.linalg.inv(Am[k:k + 6, k:k + 6])
    x = np.zeros(n)
    r = np.where(free, -gvec, 0.0)
    gnorm = math.sqrt(r @ r)
    rnorm, it = gnorm, 0
    if hist is not None:
        hist.append(rnorm / (eta * gnorm) if gnorm > 0 else 0.0)
    if rnorm <= eta * gnorm or max_it <= 0:
        return x, it, rnorm, gnorm
    z = Minv @ r
    p = z.copy()
    rz = r @ z
    while True:
        y = np.where(free, Am @ p, 0.0)
        pAp = p @ y
        if not (pAp > 0) or not math.isfinite(pAp):
            break
        a = rz / pAp
        x = x + a * p
        r = r - a * y
        rnorm = math.sqrt(r @ r)
        it += 1
        if hist is not None:
            hist.append(rnorm / (eta * gnorm))
        if rnorm <= eta * gnorm or it >= max_it:
            break
        z = Minv @ r
        rz2 = r @ z
        p = z + (rz2 / rz) * p
        rz = rz2
    return x, it, rnorm, gnorm


def apply_step(g, q, t, x):
    """candidate (q, t): q <- normalised q * exp(omega), t <- t + R(q) v with the R before the step; fixed nodes stay"""
    q2, t2 = q.copy(), t.copy()
    for n in range(g.N):
        if g.fixed[n]:
            continue
        qq = quat_mul(q[n], quat_exp(x[6 * n:6 * n + 3]))
        q2[n] = qq / math.sqrt(qq @ qq)
        t2[n] = t[n] + R_from_quat(q[n]) @ x[6 * n + 3:6 * n + 6]
    return q2, t2


def solve(g, params=None, steps=None, n_steps=None):
    """the outer loop: Levenberg-Marquardt under the trust-region policy of csrc/ba.hip.  Returns a dict with R, t, the summary fields and
    the trace rows (radius, kind, cost_change, model_cost_change, rho, candidate cost, pcg iterations).  steps, a list, receives one dict
    per trial step (what replay() documents); n_steps ends the loop after that many trial steps (termination 1)."""
    P = dict(DEFAULTS, **(params or {}))
    max_pcg = P["max_pcg_iterations"] or max(100, 2 * g.N)
    q = np.array([quat_from_R(R) for R in g.R]); t = g.t.copy()
    Rs = lambda qq: np.array([R_from_quat(v) for v in qq])
    cost, res, A, B, grad = linearize(g, Rs(q), t)
    out = dict(initial_cost=cost, termination=2, num_successful_steps=0, pcg_iterations=0, trace=[])
    free = np.repeat(g.fixed == 0, 6)
    radius, decrease, reuse, iteration, invalid = 1e4, 2.0, False, 0, 0
    D = None
    while True:
        if iteration >= P["max_iterations"] or (n_steps is not None and iteration >= n_steps):
            out["termination"] = 1; break
        if np.abs(grad[free]).max(initial=0.0) <= P["gradient_tolerance"] or radius < 1e-32:
            out["termination"] = 0; break
        iteration += 1
        J = dense_jacobian(g, A, B); H = J.T @ J
        if not reuse:
            D = lm_diagonal(H, g.fixed)
        hist = []
        x, its, _, _ = pcg(H, D, radius, grad, g.fixed, P["eta"], max_pcg, hist)
        out["pcg_iterations"] += its
        Jx = J @ x
        model = -(x @ grad + 0.5 * (Jx @ Jx))
        rec = dict(radius=radius, reuse=reuse, pcg_iterations=its, kind=0, rho=0.0, q=q, t=t, x=x, D=D, A=A, B=B, grad=grad, cost=cost,
                   pcg_margin=min(abs(h - 1) for h in hist[-2:]), rho_margin=np.inf, ftol_margin=np.inf, ptol_margin=np.inf)
        if steps is not None:
            steps.append(rec)
        if not (model > 0) or not np.isfinite(x).all():
            out["trace"].append((radius, 0, 0, model, 0, 0, its))
            invalid += 1
            if invalid >= 5:
                out["termination"] = 2; break
            radius /= decrease; decrease *= 2; reuse = False
            continue
        cq, ct = apply_step(g, q, t, x)
        cand = linearize(g, Rs(cq), ct)
        fr = g.fixed == 0
        step_norm = math.sqrt(((cq - q)[fr] ** 2).sum() + ((ct - t)[fr] ** 2).sum())
        x_norm = math.sqrt((q[fr] ** 2).sum() + (t[fr] ** 2).sum())
        change = cost - cand[0]
        p_lim, f_lim = P["parameter_tolerance"] * (x_norm + P["parameter_tolerance"]), P["function_tolerance"] * cost
        rec["ptol_margin"] = abs(step_norm / p_lim - 1) if p_lim > 0 else np.inf
        if step_norm <= p_lim:
            rec["kind"] = 3
            out["trace"].append((radius, 3, change, model, 0, cand[0], its)); out["termination"] = 0; break
        rec["ftol_margin"] = abs(abs(change) / f_lim - 1) if f_lim > 0 else np.inf
        if abs(change) <= f_lim:
            rec["kind"] = 4
            out["trace"].append((radius, 4, change, model, 0, cand[0], its)); out["termination"] = 0; break
        rho = change / model
        accept = rho > 1e-3
        rec.update(kind=1 if accept else 2, rho=rho, rho_margin=abs(rho - 1e-3) / abs(rho))
        out["trace"].append((radius, 1 if accept else 2, change, model, rho, cand[0], its))
        if accept:
            q, t = cq, ct
            cost, res, A, B, grad = cand
            out["num_successful_steps"] += 1
            invalid = 0
            radius = min(1e16, radius / max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3))
            decrease, reuse = 2.0, False
        else:
            invalid = 0
            radius /= decrease; decrease *= 2; reuse = True
    out.update(num_iterations=iteration, final_cost=cost, R=Rs(q), t=t)
    return out


def replay(g, params, n_steps):
    """the first n_steps trial steps of solve(g, params), one dict each: the restatement's radius, reuse (the LM diagonal is kept), pcg_iterations,
    kind and rho; what the step started from (q, t, cost, the blocks A, B, grad, the diagonal D) and its step x; and how far each decision
    was from its threshold: pcg_margin, the smaller |rnorm / (eta gnorm) - 1| of the stopping PCG iteration and the one before it;
    rho_margin |rho - 1e-3| / |rho|; ftol_margin and ptol_margin, |lhs / rhs - 1| of the two tolerance comparisons (inf where a
    comparison was not reached)."""
    steps = []
    solve(g, params, steps=steps, n_steps=n_steps)
    return steps


def _edge_product(g, A, B, v):
    """u_e = A_e v_i + B_e v_j, [E][6]"""
    v = v.reshape(-1, 6)
    return np.einsum("eab,eb->ea", A, v[g.ei]) + np.einsum("eab,eb->ea", B, v[g.ej])


def _inv6(M):
    """inverses of [n][6][6] blocks by Gauss-Jordan without pivoting (the blocks are positive definite), in the blocks' number type"""
    n = len(M)
    W = np.concatenate([M.copy(), np.broadcast_to(np.eye(6, dtype=M.dtype), (n, 6, 6)).copy()], axis=2)
    for c in range(6):
        W[:, c, :] = W[:, c, :] / W[:, c, c][:, None]
        for r in range(6):
            if r != c:
                W[:, r, :] = W[:, r, :] - W[:, r, c][:, None] * W[:, c, :]
    return W[:, :, 6:]


def pcg_k(g, A, B, D, radius, gvec, k, dtype=np.longdouble):
    """x after exactly k iterations of pcg()'s recurrence on (J^T J + D / radius) x = -g, in `dtype` and without the dense matrices: J p
    per edge, J^T of that per node.  What the step tests hold a float64 PCG stopped at iteration k against."""
    A, B, D, gvec = (np.asarray(a, dtype) for a in (A, B, D, gvec))
    N = g.N
    free = np.repeat(g.fixed == 0, 6)

    def scatter(U, out):     # out_n += sum over the edges at n of (A_e or B_e)^T U_e
        np.add.at(out, g.ei, np.einsum("eab,ea->eb", A, U))
        np.add.at(out, g.ej, np.einsum("eab,ea->eb", B, U))
        return out

    def op(p):
        y = scatter(_edge_product(g, A, B, p), np.zeros((N, 6), dtype)).ravel() + (D / dtype(radius)) * p
        return np.where(free, y, 0)
    Hd = np.zeros((N, 6, 6), dtype)
    np.add.at(Hd, g.ei, np.einsum("eab,eac->ebc", A, A))
    np.add.at(Hd, g.ej, np.einsum("eab,eac->ebc", B, B))
    Hd = Hd + (D / dtype(radius)).reshape(N, 6)[:, :, None] * np.eye(6, dtype=dtype)
    fixed = g.fixed != 0
    Hd[fixed] = np.eye(6, dtype=dtype)
    Minv = _inv6(Hd)
    Minv[fixed] = 0
    pre = lambda r: np.einsum("nab,nb->na", Minv, r.reshape(N, 6)).ravel()
    x = np.zeros(6 * N, dtype)
    r = np.where(free, -gvec, 0)
    if k <= 0:
        return x
    z = pre(r); p = z.copy(); rz = r @ z
    for it in range(k):
        y = op(p)
        a = rz / (p @ y)
        x = x + a * p
        r = r - a * y
        if it + 1 < k:
            z = pre(r); rz2 = r @ z
            p = z + (rz2 / rz) * p
            rz = rz2
    return x


def pcg_distance(x, want):
    want = np.asarray(want, np.longdouble)
    return float(np.sqrt(((np.asarray(x, np.longdouble) - want) ** 2).sum()) / np.sqrt((want ** 2).sum()))


def trial_step(g, q, t, x, lin=None, dtype=np.longdouble):
    """what ONE trial produces from a given step x at the poses (q [N][4], t [N][3]), in `dtype`: the candidate poses (cand_q, cand_t), the
    candidate's cost, x.g (xg), |J x|^2 / 2 (half_m), the model cost change -(x.g + |J x|^2 / 2), step2 = |candidate - point|^2 and
    x2 = |point|^2 over the free nodes.  lin: linearize()'s tuple at the poses, made here when not given.  A step entry on a fixed node
    is not read."""
    q = np.asarray(q, dtype); t = np.asarray(t, dtype); x = np.asarray(x, dtype)
    Rs = lambda qq: np.array([R_from_quat(v) for v in qq])
    if lin is None:
        lin = linearize(g, Rs(q), t, dtype=dtype)
    _, _, A, B, grad = (np.asarray(a, dtype) for a in lin)
    cq, ct = q.copy(), t.copy()
    step2 = x2 = dtype(0)
    half = dtype(1) / 2
    xf = x.reshape(-1, 6) * (g.fixed == 0)[:, None].astype(dtype)
    for n in range(g.N):
        if g.fixed[n]:
            continue
        w, v = xf[n, :3], xf[n, 3:]
        th = np.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
        if th == 0:
            e = np.array([1, 0, 0, 0], dtype)
        else:
            s = np.sin(th * half) / th
            e = np.array([np.cos(th * half), s * w[0], s * w[1], s * w[2]], dtype)
        qq = quat_mul(q[n], e)
        cq[n] = qq / np.sqrt(qq @ qq)
        ct[n] = t[n] + R_from_quat(q[n]) @ v
        step2 = step2 + ((cq[n] - q[n]) ** 2).sum() + ((ct[n] - t[n]) ** 2).sum()
        x2 = x2 + (q[n] ** 2).sum() + (t[n] ** 2).sum()
    cand_cost = linearize(g, Rs(cq), ct, dtype=dtype)[0]
    u = _edge_product(g, A, B, xf.ravel())
    xg, half_m = xf.ravel() @ grad, (u * u).sum() * half
    return dict(cand_q=cq, cand_t=ct, cand_cost=cand_cost, xg=xg, half_m=half_m, model_cost_change=-(xg + half_m), step2=step2, x2=x2)


def trial_distance(g, got, want):
    """the distance TRIAL_MEASURED is stated in, per quantity, the largest of them.  `want`: trial_step() in longdouble; `got`: a dict with
    cand_q, cand_t, cand_cost, model_cost_change, step2, x2.  Candidate poses: absolute, against 1 and max(1, |t|_max).  The candidate's
    cost: against lin_distance's scale for a cost.  The model change: against |x.g| + |J x|^2 / 2, the terms that cancel in it.
    step2 and x2: against their own values."""
    L = np.longdouble
    s_r = float(max(g.w_rot.max(), g.w_trans.max()) * max(1.0, np.abs(want["cand_t"]).max()))
    d = dict(cand_q=np.abs(np.asarray(got["cand_q"], L) - want["cand_q"]).max(),
             cand_t=np.abs(np.asarray(got["cand_t"], L) - want["cand_t"]).max() / max(1.0, float(np.abs(want["cand_t"]).max())),
             cand_cost=abs(L(got["cand_cost"]) - want["cand_cost"]) / max(float(want["cand_cost"]), s_r * s_r),
             model=abs(L(got["model_cost_change"]) - want["model_cost_change"]) / (abs(want["xg"]) + want["half_m"]),
             step2=abs(L(got["step2"]) - want["step2"]) / want["step2"], x2=abs(L(got["x2"]) - want["x2"]) / want["x2"])
    return max(float(v) for v in d.values()), {k: float(v) for k, v in d.items()}


def verdict(rec, x_cost, params):
    """the host's rule of dvs_pgo_solve on one status record: (kind, cost change, relative decrease) — kind 0 invalid, 1 accepted,
    2 rejected, 3 parameter tolerance, 4 function tolerance; x_cost is the cost of the point the step was taken from"""
    P = dict(DEFAULTS, **(params or {}))
    if not rec["finite"] or not (rec["model_cost_change"] > 0.0):
        return 0, 0.0, 0.0
    change = x_cost - rec["cand_cost"]
    if math.sqrt(rec["step2"]) <= P["parameter_tolerance"] * (math.sqrt(rec["x2"]) + P["parameter_tolerance"]):
        return 3, change, 0.0
    if abs(change) <= P["function_tolerance"] * x_cost:
        return 4, change, 0.0
    rho = change / rec["model_cost_change"]
    return (1 if rho > 1e-3 else 2), change, rho


def trace_row(rec, radius, x_cost, params):
    """the row dvs_pgo_solve logs for the record"""
    kind, change, rho = verdict(rec, x_cost, params)
    if kind == 0:
        return [radius, 0.0, 0.0, rec["model_cost_change"], 0.0, 0.0, float(rec["pcg_iterations"])]
    return [radius, float(kind), change, rec["model_cost_change"], rho, rec["cand_cost"], float(rec["pcg_iterations"])]


def correct_points(xyz, anchor, R0, t0, R1, t1):
    """x' = R'_a (R_a^T (x - t_a)) + t'_a in float64, term after term in that order, rounded to float once"""
    xyz = np.asarray(xyz, dtype=np.float32)
    out = xyz.copy()
    N = len(R0)
    for k in range(len(xyz)):
        a = int(anchor[k])
        if a < 0 or a >= N:
            continue
        d = [np.float64(xyz[k, c]) - t0[a, c] for c in range(3)]
        y = [R0[a, 0, c] * d[0] + R0[a, 1, c] * d[1] + R0[a, 2, c] * d[2] for c in range(3)]
        for c in range(3):
            out[k, c] = np.float32(R1[a, c, 0] * y[0] + R1[a, c, 1] * y[1] + R1[a, c, 2] * y[2] + t1[a, c])
    return out


# ---------------------------------------------------------------------------------------------------------------- scipy's statement
def jr(phi):
    th = math.sqrt(phi @ phi)
    W = hat(phi)
    if th < 1e-6:
        return np.eye(3) - W / 2 + (W @ W) / 6
    return np.eye(3) - (1 - math.cos(th)) / th ** 2 * W + (th - math.sin(th)) / th ** 3 * (W @ W)


def scipy_solve(g):
    """scipy.optimize.least_squares on the stated residual over (rotation vector, t) of the free nodes, exact trust-region solver.  Its
    Jacobian is the rule's blocks times d delta / d (phi, t) = blockdiag(Jr(phi), R^T) — checked against central differences on the CPU."""
    from scipy.optimize import least_squares
    from scipy.spatial.transform import Rotation
    free = np.flatnonzero(g.fixed == 0)
    cols = np.concatenate([np.arange(6 * n, 6 * n + 6) for n in free]) if len(free) else np.zeros(0, int)

    def unpack(x):
        R, t = g.R.copy(), g.t.copy()
        for k, n in enumerate(free):
            R[n] = Rotation.from_rotvec(x[6 * k:6 * k + 3]).as_matrix(); t[n] = x[6 * k + 3:6 * k + 6]
        return R, t

    def fun(x):
        return residual_vector(g, *unpack(x))

    def jac(x):
        R, t = unpack(x)
        _, _, A, B, _ = linearize(g, R, t)
        J = dense_jacobian(g, A, B)[:, cols]
        for k, n in enumerate(free):
            T = np.zeros((6, 6)); T[:3, :3] = jr(x[6 * k:6 * k + 3]); T[3:, 3:] = R[n].T
            J[:, 6 * k:6 * k + 6] = J[:, 6 * k:6 * k + 6] @ T
        return J

    x0 = np.concatenate([np.concatenate([Rotation.from_matrix(g.R[n]).as_rotvec(), g.t[n]]) for n in free])
    sol = least_squares(fun, x0, jac=jac, method="trf", xtol=1e-15, ftol=1e-15, gtol=1e-12, max_nfev=200)
    R, t = unpack(sol.x)
    return dict(cost=float(sol.cost), R=R, t=t, nfev=int(sol.nfev), fun=fun, jac=jac, x0=x0)


@functools.lru_cache(maxsize=None)
def scipy_cost(name):
    return scipy_solve(graph(name))["cost"]


# ---------------------------------------------------------------------------------------------------------------- graphs
def _planted(N):
    """a double loop: two turns of a circle of radius 5 m that rises 0.3 m per turn, the camera turning with the path and nodding"""
    R, t = [], []
    for k in range(N):
        a = 4 * math.pi * k / N
        t.append([5 * math.cos(a), 5 * math.sin(a), 0.3 * a / (2 * math.pi)])
        R.append(rodrigues(np.array([0.0, 0.0, a + math.pi / 2])) @ rodrigues(np.array([0.2 * math.sin(3 * a), 0.1 * math.cos(2 * a), 0.0])))
    return np.array(R), np.array(t)


def _measure(R, t, i, j, rng, s_rot, s_trans):
    """Z ~ T_i^-1 T_j with noise: (rvec, tvec)"""
    Rz = R[i].T @ R[j]
    tz = R[i].T @ (t[j] - t[i])
    if s_rot > 0:
        Rz = Rz @ rodrigues(rng.normal(0, s_rot, 3)); tz = tz + rng.normal(0, s_trans, 3)
    w, _ = so3_log(Rz)
    # Log's own precision near pi is not at stake here (relative rotations of these graphs stay below 3 rad); refine once
    Rw = rodrigues(w)
    w = w + so3_log(Rw.T @ Rz)[0]
    return w, tz


def make_graph(N, loops, extra=(), seed=0, noise=True):
    rng = np.random.default_rng(seed)
    R, t = _planted(N)
    so, to, sl, tl = (0.01, 0.02, 0.003, 0.005)
    ei, ej, rv, tv, wr, wt = [], [], [], [], [], []
    for i in range(N - 1):
        w, z = _measure(R, t, i, i + 1, rng, so if noise else 0, to)
        ei.append(i); ej.append(i + 1); rv.append(w); tv.append(z); wr.append(1 / so); wt.append(1 / to)
    for (i, j) in list(loops) + list(extra):
        w, z = _measure(R, t, i, j, rng, sl if noise else 0, tl)
        ei.append(i); ej.append(j); rv.append(w); tv.append(z); wr.append(1 / sl); wt.append(1 / tl)
    # initial poses: the odometry chained from node 0 — with noise-free measurements the chain would BE the planted poses, so `exact`
    # graphs chain the noisy odometry of the same seed instead and keep the exact measurements as edges
    rng2 = np.random.default_rng(seed + 1000)
    R0, t0 = [R[0]], [t[0]]
    for i in range(N - 1):
        if noise:
            Rz, tz = rodrigues(rv[i]), tv[i]
        else:
            w, tz = _measure(R, t, i, i + 1, rng2, so, to); Rz = rodrigues(w)
        t0.append(t0[i] + R0[i] @ tz); R0.append(R0[i] @ Rz)
    fixed = np.zeros(N, np.uint8); fixed[0] = 1
    return Graph(np.array(R0), np.array(t0), fixed, ei, ej, rv, tv, wr, wt, planted=(R, t))


def _hub_extra():
    rng = np.random.default_rng(77)
    others = [n for n in range(300) if abs(n - 150) > 1]
    return [(150, int(n)) for n in rng.choice(others, 70, replace=False)]


@functools.lru_cache(maxsize=None)
def graph(name):
    if name == "ring24":
        return make_graph(24, [(23, 0), (22, 1), (12, 0)], seed=1)
    if name == "exact24":
        return make_graph(24, [(23, 0), (22, 1), (12, 0)], seed=1, noise=False)
    if name == "hub300":
        return make_graph(300, [(299, 0), (150, 1)], _hub_extra(), seed=2)
    if name == "ring24_far":
        return _far(1.0, 2.0, 3)
    if name == "ring24_far2":
        return _far(2.0, 5.0, 4)
    if name == "chain515":
        return make_graph(515, [(514, 0), (257, 1), (400, 100)], seed=3)
    if name == "chain515_fixed":
        g = make_graph(515, [(514, 0), (257, 1), (400, 100)], seed=3)
        g.fixed[513] = 1
        return g
    return edge_case(name)


def _far(s_rot, s_trans, seed):
    """ring24 started far from its minimum: nodes 1 .. 23 moved by R_n <- R_n Exp(N(0, s_rot)^3), t_n += N(0, s_trans)^3, node after node"""
    g = graph("ring24")
    rng = np.random.default_rng(seed)
    R, t = g.R.copy(), g.t.copy()
    for n in range(1, g.N):
        R[n] = R[n] @ rodrigues(rng.normal(0, s_rot, 3)); t[n] = t[n] + rng.normal(0, s_trans, 3)
    return Graph(R, t, g.fixed, g.ei, g.ej, g.rvec, g.tvec, g.w_rot, g.w_trans, planted=g.planted)


# The graphs of the step tests (tests/test_pose_graph_steps_cpu.py asserts every statement here on the restatement):
#   ring24_far   kinds of the first twelve trial steps under TIGHT: FAR_KINDS — four rejections in a row (the radius divided by 2, 4, 8, 16,
#                the LM diagonal kept, a second, third .. trial from one linearisation) and a later single one
#   ring24_far2  a rejection directly after the first accepted step; the run meets the iteration limit (termination 1)
#   chain515     N = 515, E = 517: the single-workgroup loops (512 threads) make a second trip of 3 nodes and 5 edges
#   chain515_fixed  the same with a fixed node inside the second trip
#   ring24 under PTOL ends by the parameter tolerance (kind 3); overflow6 (weights 1e150) fails after five invalid steps (kind 0)
FAR_KINDS = (1, 1, 1, 1, 2, 2, 2, 2, 1, 1, 2, 1)
FAR2_KINDS = (1, 2, 2, 2, 2, 1)
PTOL = dict(TIGHT, parameter_tolerance=1e-3, function_tolerance=1e-14)
OVERFLOW_RADII = (1e4, 5e3, 1250.0, 156.25, 9.765625)
# (graph, parameters, replayed trial steps): the hook is driven through these steps one at a time
REPLAY_CASES = {"ring24_far": ("ring24_far", TIGHT, 15), "ring24_far2": ("ring24_far2", TIGHT, 8), "chain515": ("chain515", TIGHT, 3),
                "hub300": ("hub300", TIGHT, 3)}
# whole solves: (graph, parameters)
SOLVE_CASES = {"ring24_far": ("ring24_far", TIGHT), "ring24_far2": ("ring24_far2", TIGHT), "chain515": ("chain515", TIGHT), "ring24_ptol": ("ring24", PTOL)}
PREMISE = 1e-6


@functools.lru_cache(maxsize=None)
def replay_case(name):
    gname, params, n = REPLAY_CASES[name]
    return replay(graph(gname), params, n)


@functools.lru_cache(maxsize=None)
def solve_case(name):
    """the restatement's whole solve of a SOLVE_CASES entry, with its per-step records under "steps" """
    gname, params = SOLVE_CASES[name]
    steps = []
    out = solve(graph(gname), params, steps=steps)
    out["steps"] = steps
    return out


SOLVE_GRAPHS = ("ring24", "hub300", "exact24")
EDGE_CASES = ("two_nodes", "isolated", "duplicate", "zero_rot", "tiny_rot", "big_rot", "two_fixed")
ALL_GRAPHS = SOLVE_GRAPHS + EDGE_CASES


def edge_case(name):
    base = make_graph(6, [(5, 0)], seed=5)
    R, t, fixed = base.R.copy(), base.t.copy(), base.fixed.copy()
    ei, ej, rv, tv = list(base.ei), list(base.ej), list(base.rvec), list(base.tvec)
    wr, wt = list(base.w_rot), list(base.w_trans)
    if name == "two_nodes":
        R, t, fixed = R[:2], t[:2], fixed[:2]
        ei, ej, rv, tv, wr, wt = ei[:1], ej[:1], rv[:1], tv[:1], wr[:1], wt[:1]
    elif name == "isolated":              # node 6: free, no edge
        R = np.concatenate([R, R[:1]]); t = np.concatenate([t, t[:1] + 1.0]); fixed = np.append(fixed, 0).astype(np.uint8)
    elif name == "duplicate":
        ei.append(ei[2]); ej.append(ej[2]); rv.append(rv[2]); tv.append(tv[2]); wr.append(wr[2]); wt.append(wt[2])
    elif name in ("zero_rot", "tiny_rot", "big_rot"):
        # an extra edge (1, 3) whose rotation error at the initial poses is exactly 0 / about 1e-9 rad / about 3.0 rad: R_z = M Exp(-err)
        M = R[1].T @ R[3]
        err = dict(zero_rot=0.0, tiny_rot=1e-9, big_rot=3.0)[name]
        Rz = M if err == 0 else M @ rodrigues(np.array([0.6, -0.48, 0.64]) * -err)
        w = so3_log(Rz)[0]; w = w + so3_log(rodrigues(w).T @ Rz)[0]
        if name == "zero_rot":            # make R_z^T M the identity to the last bit: the measurement IS identity, nodes 1 and 3 share R
            R[3] = R[1]; w = np.zeros(3)
        ei.append(1); ej.append(3); rv.append(w); tv.append(R[1].T @ (t[3] - t[1])); wr.append(300.0); wt.append(200.0)
    elif name == "two_fixed":
        fixed[3] = 1
    elif name == "overflow6":             # every weight 1e150: cost (4.47e298) and gradient are finite, the gradient's squared norm is not
        wr = [1e150] * len(wr); wt = [1e150] * len(wt)
    else:
        raise KeyError(name)
    return Graph(R, t, fixed, ei, ej, rv, tv, wr, wt, planted=None)
