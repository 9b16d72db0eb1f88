"""Float64 statements of the stages of the library's own robust estimators (csrc/ransac.hip: dvs_find_fundamental_ransac*,
dvs_solve_pnp_ransac*), one function per stage, for tests/test_gpu_ransac_stages.py.  Plain numpy and Python integers, no ctypes; each
function is written from the stage's DEFINITION (the sampler rule stated in DESIGN.md, Hartley's normalised 8-point algorithm,
OpenCV's published error measures and RANSACUpdateNumIters, Grunert's three cosine-law equations), not from the kernels: where a
kernel eliminates, this file takes an SVD; where the kernel solves a quartic in closed form, this file asks np.roots.
tests/test_ransac_stage_ref_cpu.py checks these functions before any kernel is held to them."""
import math
import sys
import numpy as np

_M64 = (1 << 64) - 1
_GOLDEN = 0x9E3779B97F4A7C15
_DBL_MIN = sys.float_info.min


def splitmix64(x):
    x = (x + _GOLDEN) & _M64
    z = x
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def sample(seed, h, n, k):
    """the k indices of hypothesis h: draw j is the r-th index not drawn before (ascending), r = splitmix64(seed + golden (16 h + j + 1)) mod (n - j)"""
    left = list(range(n))
    out = []
    for j in range(k):
        r = splitmix64((seed + _GOLDEN * (16 * h + j + 1)) & _M64) % (n - j)
        out.append(left.pop(r))
    return out


def _hartley(p):
    c = p.mean(0)
    d = np.sqrt(((p - c) ** 2).sum(1)).mean()
    if not d > 0:
        return None
    s = math.sqrt(2.0) / d
    return np.array([[s, 0, -s * c[0]], [0, s, -s * c[1]], [0, 0, 1.0]])


def eight_point(p1, p2):
    """normalised 8-point algorithm, x2^T F x1 = 0: (F of unit Frobenius norm, sigma8 / sigma1 of the 8 x 9 system), or (None, 0.0)
    where the points of an image coincide or the system has no one-dimensional null space"""
    p1 = np.asarray(p1, np.float64); p2 = np.asarray(p2, np.float64)
    T1 = _hartley(p1); T2 = _hartley(p2)
    if T1 is None or T2 is None:
        return None, 0.0
    q1 = np.c_[p1, np.ones(len(p1))] @ T1.T
    q2 = np.c_[p2, np.ones(len(p2))] @ T2.T
    A = np.einsum("ni,nj->nij", q2, q1).reshape(len(p1), 9)
    _, s, Vt = np.linalg.svd(A)
    if len(s) < 8 or not s[7] > 1e-13 * s[0]:
        return None, 0.0
    Fn = Vt[8].reshape(3, 3)
    U, d, Wt = np.linalg.svd(Fn)
    Fn = U @ np.diag([d[0], d[1], 0.0]) @ Wt
    F = T2.T @ Fn @ T1
    nrm = np.linalg.norm(F)
    if not (nrm > 0 and np.isfinite(nrm)):
        return None, 0.0
    return F / nrm, float(s[7] / s[0])


def epipolar_error(F, p1, p2):
    """per correspondence: the larger of the two squared point-to-epipolar-line distances (OpenCV's FMEstimatorCallback::computeError)"""
    F = np.asarray(F, np.float64).reshape(3, 3)
    x1 = np.c_[np.asarray(p1, np.float64), np.ones(len(p1))]
    x2 = np.c_[np.asarray(p2, np.float64), np.ones(len(p2))]
    l2 = x1 @ F.T                                   # lines in image 2
    l1 = x2 @ F                                     # lines in image 1
    with np.errstate(divide="ignore", invalid="ignore"):
        e2 = (x2 * l2).sum(1) ** 2 / (l2[:, 0] ** 2 + l2[:, 1] ** 2)
        e1 = (x1 * l1).sum(1) ** 2 / (l1[:, 0] ** 2 + l1[:, 1] ** 2)
    return np.fmax(e1, e2)


def reprojection_error2(R, t, K4, X, uv):
    """squared reprojection error of x = K (R X + t); a point with depth z <= 1e-9 gets +inf: it is never an inlier"""
    Xc = np.asarray(X, np.float64) @ np.asarray(R, np.float64).reshape(3, 3).T + np.asarray(t, np.float64)
    z = Xc[:, 2]
    ok = z > 1e-9
    zs = np.where(ok, z, 1.0)
    du = K4[0] * Xc[:, 0] / zs + K4[2] - np.asarray(uv, np.float64)[:, 0]
    dv = K4[1] * Xc[:, 1] / zs + K4[3] - np.asarray(uv, np.float64)[:, 1]
    return np.where(ok, du * du + dv * dv, np.inf)


def update_num_iters(p, ep, model_points, max_iters):
    """cv::RANSACUpdateNumIters -> (iterations, num / denom before rounding or None where no rounding takes place)"""
    p = min(max(p, 0.0), 1.0); ep = min(max(ep, 0.0), 1.0)
    num = max(1.0 - p, _DBL_MIN)
    denom = 1.0 - (1.0 - ep) ** model_points
    if denom < _DBL_MIN:
        return 0, None
    num = math.log(num); denom = math.log(denom)
    if denom >= 0 or -num >= max_iters * (-denom):
        return max_iters, None
    q = num / denom
    return int(round(q)), q                          # round(): half to even, as rint() — the callers keep q away from half-integers


def replay_select(counts, n, model_points, confidence, group):
    """the sequential RANSAC loop over precomputed counts: iteration `it` offers models it * group .. it * group + group - 1 in order, a
    count above max(best so far, model_points - 1) becomes the best and resets the iteration limit.  Returns (best or -1, iterations run,
    best count, smallest distance of any rounded quotient to a half-integer — inf when none was rounded)."""
    counts = [int(c) for c in counts]
    max_iters = len(counts) // group
    niters, best, best_count, it, margin = max_iters, -1, 0, 0, math.inf
    while it < niters and it < max_iters:
        for s in range(group):
            h = it * group + s
            if counts[h] > max(best_count, model_points - 1):
                best_count, best = counts[h], h
                niters, q = update_num_iters(confidence, (n - counts[h]) / n, model_points, max_iters)
                if q is not None:
                    margin = min(margin, abs(q - math.floor(q) - 0.5))
        it += 1
    return best, it, best_count, margin


def p3p_roots(P, j):
    """Grunert's P3P for object points P (3 x 3, rows) seen along unit bearings j (rows).  With depths s1, s2 = u s1, s3 = v s1 the three
    cosine laws  s_a^2 + s_b^2 - 2 s_a s_b cos(j_a, j_b) = |P_a - P_b|^2  give, after dividing out s1^2, two quadratics in u whose
    coefficients are polynomials in v; their resultant is the quartic in v.  Returns (admissible [(v, u)] in ascending v — real v > 0 with
    u > 0 —, smallest pairwise distance between the quartic's four roots relative to max(1, |root|): the conditioning gate)."""
    from numpy.polynomial import Polynomial as Poly
    P = np.asarray(P, np.float64); j = np.asarray(j, np.float64)
    a2 = ((P[1] - P[2]) ** 2).sum(); b2 = ((P[0] - P[2]) ** 2).sum(); c2 = ((P[0] - P[1]) ** 2).sum()
    ca = j[1] @ j[2]; cb = j[0] @ j[2]; cg = j[0] @ j[1]
    v = Poly([0.0, 1.0])
    m13 = 1.0 + v * v - 2.0 * cb * v                 # |s1 j1 - s3 j3|^2 / s1^2 = b2 / s1^2
    # (1 + u^2 - 2 u cg) b2 = c2 m13      and      (u^2 + v^2 - 2 u v ca) b2 = a2 m13, as p2 u^2 + p1 u + p0 and q2 u^2 + q1 u + q0
    p2, p1, p0 = Poly([b2]), Poly([-2.0 * b2 * cg]), Poly([b2]) - c2 * m13
    q2, q1, q0 = Poly([b2]), -2.0 * b2 * ca * v, b2 * v * v - a2 * m13
    res = (p2 * q0 - p0 * q2) ** 2 - (p2 * q1 - p1 * q2) * (p1 * q0 - p0 * q1)
    co = res.coef
    co = np.concatenate([co, np.zeros(5 - len(co))]) if len(co) < 5 else co
    roots = np.roots(co[::-1] / np.abs(co).max())
    if len(roots) < 4:
        return [], 0.0
    sep = min(abs(roots[a] - roots[b]) / max(1.0, abs(roots[a]), abs(roots[b])) for a in range(4) for b in range(a))
    out = []
    for r in sorted(roots, key=lambda z: z.real):
        if abs(r.imag) > 1e-9 * max(1.0, abs(r)) or not r.real > 0:
            continue
        vv = r.real
        den = q1(vv) - p1(vv)                        # the difference of the two quadratics is linear in u
        if den == 0:
            continue
        uu = (p0(vv) - q0(vv)) / den
        if uu > 0:
            out.append((vv, uu))
    return out, float(sep)


def rodrigues(R):
    """rotation matrix -> principal Rodrigues vector, through the axis: the eigenvector of eigenvalue 1"""
    R = np.asarray(R, np.float64).reshape(3, 3)
    w, V = np.linalg.eig(R)
    a = V[:, np.argmin(np.abs(w - 1.0))].real
    a = a / np.linalg.norm(a)
    s = 0.5 * (np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) @ a)
    c = 0.5 * (np.trace(R) - 1.0)
    th = math.atan2(s, c)
    return a * th                                    # (-a, -th) is the same vector: the sign of the eigenvector does not matter


def _counts(H, **at):
    c = [0] * H
    for k, v in at.items():
        c[int(k[1:])] = v
    return c


# Hand-made count vectors for the select stage, n = 100 correspondences, confidence 0.99; `expect` = (best, iterations run, best count),
# worked out by hand from RANSACUpdateNumIters: ln(0.01) / ln(1 - w^m) with w the inlier share and m the model size gives
#   m = 3: w = 0.90 -> 3.527 -> 4,  w = 0.95 -> 2.365 -> 2;     m = 8: w = 0.80 -> 25.08 -> 25,  w = 0.85 -> 14.48 -> 14;
# a share of 0.5 or 0.6 asks for more iterations than any vector here has, so the limit stays; w = 1 gives 0: the loop ends at once.
SELECT_CASES = [
    dict(name="all zeros", counts=_counts(50), model_points=8, group=1, expect=(-1, 50, 0)),
    dict(name="model_points - 1 is ignored", counts=_counts(50, i3=7, i10=8), model_points=8, group=1, expect=(10, 50, 8)),
    dict(name="only model_points - 1", counts=_counts(50, i3=7), model_points=8, group=1, expect=(-1, 50, 0)),
    dict(name="equal counts: the first wins", counts=_counts(50, i2=50, i5=50), model_points=8, group=1, expect=(2, 50, 50)),
    dict(name="group 4: best in slot 3", counts=_counts(40, i11=60), model_points=3, group=4, expect=(11, 10, 60)),
    dict(name="group 4: equal counts within one sample", counts=_counts(40, i9=60, i11=60), model_points=3, group=4, expect=(9, 10, 60)),
    dict(name="count == n ends the loop", counts=_counts(50, i4=100, i5=100), model_points=8, group=1, expect=(4, 5, 100)),
    dict(name="group 4: count == n ends the loop after its sample", counts=_counts(40, i9=100), model_points=3, group=4, expect=(9, 3, 100)),
    dict(name="early stop, better one before", counts=_counts(200, i0=90, i3=95), model_points=3, group=1, expect=(3, 4, 95)),
    dict(name="early stop, better at the stop", counts=_counts(200, i0=90, i4=95), model_points=3, group=1, expect=(0, 4, 90)),
    dict(name="early stop, better one after", counts=_counts(200, i0=90, i5=95), model_points=3, group=1, expect=(0, 4, 90)),
    dict(name="early stop m = 8, better one before", counts=_counts(200, i0=80, i24=85), model_points=8, group=1, expect=(24, 25, 85)),
    dict(name="early stop m = 8, better at the stop", counts=_counts(200, i0=80, i25=85), model_points=8, group=1, expect=(0, 25, 80)),
    dict(name="early stop m = 8, better one after", counts=_counts(200, i0=80, i26=85), model_points=8, group=1, expect=(0, 25, 80)),
    dict(name="group 4 early stop, better one before", counts=_counts(160, i1=90, i14=95), model_points=3, group=4, expect=(14, 4, 95)),
    dict(name="group 4 early stop, better at the stop", counts=_counts(160, i1=90, i16=95), model_points=3, group=4, expect=(1, 4, 90)),
    dict(name="H = 1", counts=[50], model_points=8, group=1, expect=(0, 1, 50)),
    dict(name="H = 1, nothing", counts=[7], model_points=8, group=1, expect=(-1, 1, 0)),
]
SELECT_N, SELECT_CONFIDENCE = 100, 0.99
