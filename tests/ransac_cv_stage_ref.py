"""Float64 statements of the stages of the OpenCV-procedure robust estimators (csrc/ransac.hip, csrc/pnp_cv.h: dvs_find_fundamental_cv*,
dvs_solve_pnp_ransac_cv*), one function per stage, for tests/test_gpu_ransac_cv_stages.py.  Plain numpy (scipy for the one optimisation),
no ctypes; each function is written from the stage's DEFINITION — the 7-point algorithm, OpenCV's published error measures, loop rules
and initialisations, the EPnP paper — not from the kernels and not from oracle/*.cpp: where a kernel eliminates or runs a Jacobi
eigen-decomposition of a normal matrix, this file takes an SVD of the system itself; where the kernel solves a cubic in closed form, this
file interpolates the determinant and asks np.roots.  tests/test_ransac_cv_stage_ref_cpu.py checks these functions before any kernel is
held to them."""
import math
import numpy as np
from ransac_stage_ref import epipolar_error, rodrigues, update_num_iters   # noqa: F401  (shared with the own estimators' statements)

SAME_POSE = 1e-6   # two of EPnP's three candidates within this of each other (R and t entries) are one pose
BAND_F = 1e-6   # float32 rounding of an error and of the threshold is 6e-8 relative each: a factor of 16 to spare


# ------------------------------------------------------------------ fundamental matrix
def seven_point(p1, p2, idx):
    """the 7-point algorithm on correspondences idx (x2^T F x1 = 0, raw pixel coordinates): the null space of the 7 x 9 system from its
    SVD, det(l f1 + (1 - l) f2) = 0 as a cubic interpolated at four l, one model per real root scaled to F[2, 2] = 1.
    Returns (models — a SET, in no particular order: the order follows the null-space basis —, sigma7 / sigma1 of the system, smallest
    distance between two of the cubic's three roots relative to max(1, |root|))."""
    a = np.asarray(p1, np.float64)[list(idx)]; b = np.asarray(p2, np.float64)[list(idx)]
    x1 = np.c_[a, np.ones(7)]; x2 = np.c_[b, np.ones(7)]
    A = np.einsum("ni,nj->nij", x2, x1).reshape(7, 9)
    _, s, Vt = np.linalg.svd(A)
    f1, f2 = Vt[7].reshape(3, 3), Vt[8].reshape(3, 3)
    ls = np.array([-1.0, 0.0, 1.0, 2.0])
    dets = np.array([np.linalg.det(l * f1 + (1 - l) * f2) for l in ls])
    coef = np.linalg.solve(np.vander(ls, 4), dets)             # highest power first
    if not abs(coef[0]) > 1e-14 * np.abs(coef).max():
        return [], float(s[6] / s[0]), 0.0
    roots = np.roots(coef)
    sep = min(abs(roots[i] - roots[j]) / max(1.0, abs(roots[i]), abs(roots[j])) for i in range(3) for j in range(i))
    models = []
    for r in roots:
        if abs(r.imag) > 1e-9 * max(1.0, abs(r)):
            continue
        F = r.real * f1 + (1 - r.real) * f2
        if abs(F[2, 2]) > np.finfo(np.float64).eps:
            F = F / F[2, 2]
        models.append(F)
    return models, float(s[6] / s[0]), float(sep)


def unit(F):
    F = np.asarray(F, np.float64).reshape(3, 3)
    return F / np.linalg.norm(F)


def match_sets(A, B):
    """two sets of models at unit Frobenius norm, sign aligned, matched greedily: the largest max-norm difference of the pairing, or inf
    where the sets differ in size"""
    if len(A) != len(B):
        return math.inf
    B = [unit(b) for b in B]
    worst = 0.0
    for a in A:
        a = unit(a)
        d = [min(np.abs(a - b).max(), np.abs(a + b).max()) for b in B]
        k = int(np.argmin(d))
        worst = max(worst, d[k])
        B.pop(k)
    return worst


def count_float(errors, thr2):
    """(#{e < thr2 (1 - BAND_F)}, #{e inside the band thr2 (1 +- BAND_F)}): a float32 comparison e <= thr2 counts every one of the
    first and may count any of the second"""
    e = np.asarray(errors, np.float64); t = float(thr2)
    strict = e < t * (1 - BAND_F)
    band = ~strict & (e <= t * (1 + BAND_F))
    return int(strict.sum()), int(band.sum())


def replay_select_cv(counts, n, model_points, confidence, group, found, max_iters_true):
    """RANSACPointSetRegistrator::run over precomputed counts of which only the first len(counts) // group iterations are at hand: the
    loop of up to max_iters_true iterations runs while it has models and getSubset had a sample (`found`); a count above
    max(best so far, model_points - 1) becomes the best and RANSACUpdateNumIters, capped at the limit in force, sets the new limit.
    Returns (best or -1, iterations run, best count, 1 where the loop wanted to go on past the models at hand, smallest distance of a
    rounded quotient to a half-integer)."""
    counts = [int(c) for c in counts]
    avail = len(counts) // group
    niters, best, best_count, it, margin = max_iters_true, -1, 0, 0, math.inf
    while it < niters and it < avail and it < found:
        for s in range(group):
            h = it * group + s
            if counts[h] > max(best_count, model_points - 1):
                best_count, best = counts[h], h
                niters, q = update_num_iters(confidence, (n - counts[h]) / n, model_points, niters)
                if q is not None:
                    margin = min(margin, abs(q - math.floor(q) - 0.5))
        it += 1
    unfinished = it < niters and it >= avail and found >= avail
    return best, it, best_count, int(unfinished), margin


def lmeds(F_all, valid, p1, p2, n):
    """LMeDSPointSetRegistrator::run over given models: a model's score is the upper median of its float32 errors (sorted index n // 2), the
    first strictly smaller median wins; sigma = 2.5 * 1.4826 * (1 + 5 / (n - 7)) * sqrt(median), at least 0.001; inliers are the points
    with (float)e <= (float)(sigma^2); success needs 7 of them.  Returns dict(winner (-1: none), median, thr2 = sigma^2, errors (float64,
    of the winner), count, success, medians (of every model, nan where invalid), gap = (second smallest - smallest) / smallest median)."""
    F_all = np.asarray(F_all, np.float64).reshape(-1, 9)
    med = np.full(len(F_all), np.nan)
    for m in range(len(F_all)):
        if not valid[m]:
            continue
        with np.errstate(all="ignore"):
            e = epipolar_error(F_all[m], p1[:n], p2[:n]).astype(np.float32)
        if np.isnan(e).any():
            continue
        med[m] = np.sort(e)[n // 2]
    ok = np.flatnonzero(~np.isnan(med))
    if len(ok) == 0:
        return dict(winner=-1, median=math.nan, thr2=math.nan, errors=None, count=0, success=0, medians=med, gap=math.inf)
    best = int(ok[np.argmin(med[ok])])                                       # argmin: the first of equal minima
    srt = np.sort(med[ok])
    gap = math.inf if len(srt) < 2 else (float(srt[1] - srt[0]) / float(srt[0]) if srt[0] > 0 else (math.inf if srt[1] > 0 else 0.0))
    sigma = max(2.5 * 1.4826 * (1 + 5.0 / (n - 7)) * math.sqrt(float(med[best])), 0.001)
    e = epipolar_error(F_all[best], p1[:n], p2[:n])
    count = int((e.astype(np.float32) <= np.float32(sigma * sigma)).sum())
    return dict(winner=best, median=float(med[best]), thr2=sigma * sigma, errors=e, count=count, success=int(count >= 7), medians=med, gap=gap)


# ------------------------------------------------------------------ PnP
def proj_err_float(R, t, K4, X, uv):
    """PnPRansacCallback::computeError: the projection in float64 rounded to float32, the squared distance to the float32 image point in
    float32 arithmetic; a point with z == 0 projects with 1 / z := 1"""
    Xc = np.asarray(X, np.float64) @ np.asarray(R, np.float64).reshape(3, 3).T + np.asarray(t, np.float64)
    z = Xc[:, 2]
    iz = np.where(z != 0, 1.0 / np.where(z != 0, z, 1.0), 1.0)
    px = (Xc[:, 0] * iz * K4[0] + K4[2]).astype(np.float32); py = (Xc[:, 1] * iz * K4[1] + K4[3]).astype(np.float32)
    uv = np.asarray(uv, np.float32)
    dx = uv[:, 0] - px; dy = uv[:, 1] - py
    return dx * dx + dy * dy                                                  # float32


def _nearest_rotation(A):
    U, _, Vt = np.linalg.svd(A)
    return U @ Vt


def rodrigues_to_R(w):
    """cv::Rodrigues, vector -> matrix: R = cos(theta) I + (1 - cos(theta)) r r^T + sin(theta) [r]x, r = w / theta"""
    w = np.asarray(w, np.float64)
    th = math.sqrt(float(w @ w))
    if th < np.finfo(np.float64).eps:
        return np.eye(3)
    r = w / th
    K = np.array([[0, -r[2], r[1]], [r[2], 0, -r[0]], [-r[1], r[0], 0]])
    return math.cos(th) * np.eye(3) + (1 - math.cos(th)) * np.outer(r, r) + math.sin(th) * K


def _f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def epnp5(X5, uv5, K4, signs=(1.0, 1.0, 1.0)):
    """EPnP (Lepetit, Moreno-Noguer, Fua, IJCV 2009) as OpenCV's epnp.cpp arranges it, on 5 correspondences: control points = centroid and
    the principal axes scaled by sqrt(eigenvalue / n); barycentric coordinates by pseudo-inverse; the four eigenvectors of M^T M with the
    smallest eigenvalues; the betas from the three linearisations N = 1, 2, 3, each followed by 5 Gauss-Newton steps on the six
    control-point distances; sign from the first point's depth, absolute orientation by SVD, the pose of the smallest mean
    reprojection error.  (solvePnP hands EPnP the image points normalised and rounded to float32: restated.)
    signs: an eigen-decomposition leaves the sign of each principal axis open; the eight choices are eight control-point sets, and on a
    sample without an exact rigid solution eight poses (EXPERIMENTS.md).
    Returns (rvec, tvec, relative gap between the 4th and 5th smallest eigenvalue of M^T M, relative gap between the reprojection error
    of the chosen candidate and that of the best RIVAL — another of the three whose pose differs by more than SAME_POSE; 1 without one —,
    the last Gauss-Newton step of the chosen candidate relative to its betas: 5 steps often do not converge)."""
    fx, fy, cx, cy = [float(v) for v in K4]
    pw = np.asarray(X5, np.float64).reshape(5, 3)
    uv = np.asarray(uv5, np.float64).reshape(5, 2)
    us = np.c_[_f32((uv[:, 0] - cx) / fx) * fx + cx, _f32((uv[:, 1] - cy) / fy) * fy + cy]
    c0 = pw.mean(0)
    w, V = np.linalg.eigh((pw - c0).T @ (pw - c0))                            # ascending
    cws = np.vstack([c0] + [c0 + sg * math.sqrt(max(w[k], 0.0) / 5) * V[:, k] for sg, k in zip(signs, (2, 1, 0))])
    CC = (cws[1:] - cws[0]).T                                                 # columns: the three offsets
    al = (np.linalg.pinv(CC) @ (pw - c0).T).T
    alphas = np.c_[1.0 - al.sum(1), al]
    M = np.zeros((10, 12))
    for i in range(5):
        for k in range(4):
            M[2 * i, 3 * k] = alphas[i, k] * fx; M[2 * i, 3 * k + 2] = alphas[i, k] * (cx - us[i, 0])
            M[2 * i + 1, 3 * k + 1] = alphas[i, k] * fy; M[2 * i + 1, 3 * k + 2] = alphas[i, k] * (cy - us[i, 1])
    ew, ev = np.linalg.eigh(M.T @ M)                                          # ascending: ev[:, 0 .. 3] are v1 .. v4 of the paper
    gap45 = float((ew[4] - ew[3]) / max(ew[4], np.finfo(np.float64).tiny))
    v = [ev[:, k].reshape(4, 3) for k in range(4)]
    pairs = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    dv = np.array([[v[k][a] - v[k][b] for (a, b) in pairs] for k in range(4)])                     # [4][6][3]
    bb = [(0, 0), (0, 1), (1, 1), (0, 2), (1, 2), (2, 2), (0, 3), (1, 3), (2, 3), (3, 3)]          # B11 B12 B22 B13 B23 B33 B14 B24 B34 B44
    L = np.array([[(1.0 if i == j else 2.0) * (dv[i][p] @ dv[j][p]) for (i, j) in bb] for p in range(6)])
    rho = np.array([((cws[a] - cws[b]) ** 2).sum() for (a, b) in pairs])

    def gauss_newton(betas):
        for _ in range(5):
            B = np.array([betas[i] * betas[j] for (i, j) in bb])
            J = np.zeros((6, 4))
            for c, (i, j) in enumerate(bb):
                if i == j:
                    J[:, i] += 2 * L[:, c] * betas[i]
                else:
                    J[:, i] += L[:, c] * betas[j]; J[:, j] += L[:, c] * betas[i]
            step = np.linalg.lstsq(J, rho - L @ B, rcond=None)[0]
            betas = betas + step
        return betas, float(np.linalg.norm(step) / max(np.linalg.norm(betas), np.finfo(np.float64).tiny))

    def pose(betas):
        ccs = sum(betas[k] * v[k] for k in range(4))
        pcs = alphas @ ccs
        if pcs[0, 2] < 0:
            ccs, pcs = -ccs, -pcs
        pc0, pw0 = pcs.mean(0), pw.mean(0)
        U, _, Vt = np.linalg.svd((pcs - pc0).T @ (pw - pw0))
        R = U @ Vt
        if np.linalg.det(R) < 0:
            R[2] = -R[2]
        t = pc0 - R @ pw0
        Xc = pw @ R.T + t
        ue = cx + fx * Xc[:, 0] / Xc[:, 2]; ve = cy + fy * Xc[:, 1] / Xc[:, 2]
        return R, t, float(np.sqrt((us[:, 0] - ue) ** 2 + (us[:, 1] - ve) ** 2).mean())

    cands = []
    # N = 1: B11 B12 B13 B14
    b = np.linalg.lstsq(L[:, [0, 1, 3, 6]], rho, rcond=None)[0]
    s = -1.0 if b[0] < 0 else 1.0
    b0 = math.sqrt(s * b[0])
    cands.append(np.array([b0, s * b[1] / b0, s * b[2] / b0, s * b[3] / b0]))
    # N = 2: B11 B12 B22
    b = np.linalg.lstsq(L[:, [0, 1, 2]], rho, rcond=None)[0]
    if b[0] < 0:
        be = [math.sqrt(-b[0]), math.sqrt(-b[2]) if b[2] < 0 else 0.0]
    else:
        be = [math.sqrt(b[0]), math.sqrt(b[2]) if b[2] > 0 else 0.0]
    if b[1] < 0:
        be[0] = -be[0]
    cands.append(np.array([be[0], be[1], 0.0, 0.0]))
    # N = 3: B11 B12 B22 B13 B23
    b = np.linalg.lstsq(L[:, [0, 1, 2, 3, 4]], rho, rcond=None)[0]
    if b[0] < 0:
        be = [math.sqrt(-b[0]), math.sqrt(-b[2]) if b[2] < 0 else 0.0]
    else:
        be = [math.sqrt(b[0]), math.sqrt(b[2]) if b[2] > 0 else 0.0]
    if b[1] < 0:
        be[0] = -be[0]
    cands.append(np.array([be[0], be[1], b[3] / be[0], 0.0]))
    with np.errstate(all="ignore"):
        gn = [gauss_newton(c) for c in cands]
        res = [pose(b) for b, _ in gn]
    errs = np.array([r[2] for r in res])
    k = 0
    if errs[1] < errs[0]:
        k = 1
    if errs[2] < errs[k]:
        k = 2
    # a rival is another of the three whose pose is a DIFFERENT one (two linearisations that reach the same minimum are no ambiguity)
    gap_err = 1.0
    for j in range(3):
        if j == k or not np.isfinite(errs[j]):
            continue
        if max(np.abs(res[j][0] - res[k][0]).max(), np.abs(res[j][1] - res[k][1]).max()) > SAME_POSE:
            gap_err = min(gap_err, float((errs[j] - errs[k]) / errs[j]) if errs[j] > 0 else 0.0)
    if not np.isfinite(errs[k]):
        gap_err = 0.0
    return rodrigues(res[k][0]), res[k][1], gap45, gap_err, gn[k][1]


def refit_init(X, uv, K4):
    """the initialisation of cvFindExtrinsicCameraParams2 (solvePnP, SOLVEPNP_ITERATIVE, no guess), from the definition: the object points
    are planar where W2 / W1 < 1e-3 (singular values of the centred points' scatter); planar: the plane is rotated into z = 0, the
    homography plane -> normalised image comes from the normalised DLT (centroid and mean absolute deviation per axis, both point sets
    rounded to float32 as cv::findHomography takes them; its Levenberg-Marquardt polish is NOT part of this statement), and is decomposed
    (h1, h2 scaled to unit length, h3 = h1 x h2, the nearest rotation; t = h3 * 2 / (|h1| + |h2|)); otherwise the 12-parameter DLT, its
    3 x 3 part replaced by its polar factor and the translation scaled to match.  Returns (path, rvec, tvec): path 1 planar, 2 DLT, or
    (0, None, None) with fewer than 4 points, or fewer than 6 that are not planar."""
    X = np.asarray(X, np.float64).reshape(-1, 3); uv = np.asarray(uv, np.float64).reshape(-1, 2)
    n = len(X)
    if n < 4:
        return 0, None, None
    mn = np.c_[(uv[:, 0] - K4[2]) / K4[0], (uv[:, 1] - K4[3]) / K4[1]]
    Mc = X.mean(0)
    _, W, Vt = np.linalg.svd((X - Mc).T @ (X - Mc))
    if W[2] / W[1] < 1e-3:
        Rt = Vt.copy()
        if Rt[0, 2] ** 2 + Rt[1, 2] ** 2 < 1e-10:
            Rt = np.eye(3)
        if np.linalg.det(Rt) < 0:
            Rt = -Rt
        Tt = -Rt @ Mc
        P = _f32((X @ Rt.T + Tt)[:, :2]); m = _f32(mn)
        cP, cm = P.mean(0), m.mean(0)
        sP, sm = np.abs(P - cP).sum(0), np.abs(m - cm).sum(0)
        if (np.abs(np.r_[sP, sm]) < np.finfo(np.float64).eps).any():
            return 0, None, None
        sP, sm = n / sP, n / sm
        Pn, mq = (P - cP) * sP, (m - cm) * sm
        rows = []
        for (Xp, Yp), (x, y) in zip(Pn, mq):
            rows.append([Xp, Yp, 1, 0, 0, 0, -x * Xp, -x * Yp, -x])
            rows.append([0, 0, 0, Xp, Yp, 1, -y * Xp, -y * Yp, -y])
        H0 = np.linalg.svd(np.array(rows))[2][8].reshape(3, 3)
        inv_m = np.array([[1 / sm[0], 0, cm[0]], [0, 1 / sm[1], cm[1]], [0, 0, 1]])
        nP = np.array([[sP[0], 0, -cP[0] * sP[0]], [0, sP[1], -cP[1] * sP[1]], [0, 0, 1]])
        Hm = inv_m @ H0 @ nP
        Hm = Hm / Hm[2, 2]
        h1, h2, h3 = Hm[:, 0], Hm[:, 1], Hm[:, 2]
        n1, n2 = np.linalg.norm(h1), np.linalg.norm(h2)
        h1 = h1 / n1; h2 = h2 / n2
        th = h3 * (2.0 / (n1 + n2))
        Rh = _nearest_rotation(np.c_[h1, h2, np.cross(h1, h2)])
        return 1, rodrigues(Rh @ Rt), Rh @ Tt + th
    if n < 6:
        return 0, None, None
    rows = []
    for (Xp, Yp, Zp), (x, y) in zip(X, -mn):
        rows.append([Xp, Yp, Zp, 1, 0, 0, 0, 0, x * Xp, x * Yp, x * Zp, x])
        rows.append([0, 0, 0, 0, Xp, Yp, Zp, 1, y * Xp, y * Yp, y * Zp, y])
    Pm = np.linalg.svd(np.array(rows))[2][11].reshape(3, 4)
    if np.linalg.det(Pm[:, :3]) < 0:
        Pm = -Pm
    sc = np.linalg.norm(Pm[:, :3])
    R = _nearest_rotation(Pm[:, :3])
    return 2, rodrigues(R), Pm[:, 3] * (np.linalg.norm(R) / sc)


def reprojection_residuals(x, X, uv, K4):
    Xc = np.asarray(X, np.float64) @ rodrigues_to_R(x[:3]).T + x[3:]
    return np.concatenate([K4[0] * Xc[:, 0] / Xc[:, 2] + K4[2] - uv[:, 0], K4[1] * Xc[:, 1] / Xc[:, 2] + K4[3] - uv[:, 1]])


def refit_optimum(X, uv, K4, rvec0, tvec0):
    """the minimiser of the reprojection residuals next to the given start (scipy's Levenberg-Marquardt, tolerances 1e-15) -> (rvec, tvec)"""
    from scipy.optimize import least_squares
    X = np.asarray(X, np.float64); uv = np.asarray(uv, np.float64)
    sol = least_squares(reprojection_residuals, np.concatenate([rvec0, tvec0]), args=(X, uv, K4), method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15)
    return sol.x[:3], sol.x[3:]


# ------------------------------------------------------------------ hand-made inputs of the select stage
def _counts(H, **at):
    c = [0] * H
    for k, v in at.items():
        c[int(k[1:])] = v
    return c


# n = 100 correspondences, confidence 0.99; `expect` = (best, iterations run, best count, loop wanted more), worked out by hand from
# RANSACUpdateNumIters, ln(0.01) / ln(1 - w^m) with w the inlier share and m the model size:
#   m = 7: w = 0.9 -> 7.08 -> 7,  w = 0.8 -> 19.57 -> 20,  w = 0.5 -> 587.2 -> 587;     m = 5: w = 0.9 -> 5.16 -> 5, w = 0.8 -> 11.60 -> 12
SELECT_CV_N, SELECT_CV_CONFIDENCE = 100, 0.99
SELECT_CV_CASES = [
    dict(name="ends inside the available models", counts=_counts(96, i2=90), model_points=7, group=1, found=96, max_iters=1000, expect=(2, 7, 90, 0)),
    dict(name="wants 587 of 1000 with 96 available", counts=_counts(96, i5=50), model_points=7, group=1, found=1000, max_iters=1000, expect=(5, 96, 50, 1)),
    dict(name="wants all 1000, nothing found yet", counts=_counts(96), model_points=7, group=1, found=1000, max_iters=1000, expect=(-1, 96, 0, 1)),
    dict(name="the sampler gave up before the available models end", counts=_counts(96, i5=50), model_points=7, group=1, found=40, max_iters=1000,
         expect=(5, 40, 50, 0)),
    dict(name="the sampler gave up: a better count past `found` is not seen", counts=_counts(96, i5=50, i41=90), model_points=7, group=1, found=40,
         max_iters=1000, expect=(5, 40, 50, 0)),
    dict(name="the limit shrinks to exactly the available models at the last one", counts=_counts(20, i19=80), model_points=7, group=1, found=1000,
         max_iters=1000, expect=(19, 20, 80, 0)),
    dict(name="the limit shrinks to one more than the available models", counts=_counts(19, i18=80), model_points=7, group=1, found=1000, max_iters=1000,
         expect=(18, 19, 80, 1)),
    dict(name="group 3: equal counts within one sample, the first wins", counts=_counts(288, i13=50, i14=50), model_points=7, group=3, found=96,
         max_iters=1000, expect=(13, 96, 50, 1)),
    dict(name="group 3: early stop after the sample that holds the best", counts=_counts(288, i4=90, i5=80), model_points=7, group=3, found=96,
         max_iters=1000, expect=(4, 7, 90, 0)),
    dict(name="group 3: a better model in the iteration the loop ends before", counts=_counts(288, i4=90, i21=95), model_points=7, group=3, found=96,
         max_iters=1000, expect=(4, 7, 90, 0)),
    dict(name="model_points - 1 is ignored", counts=_counts(96, i3=6, i10=7), model_points=7, group=1, found=96, max_iters=96, expect=(10, 96, 7, 0)),
    dict(name="all zeros, every iteration available", counts=_counts(96), model_points=7, group=1, found=96, max_iters=96, expect=(-1, 96, 0, 0)),
    dict(name="m = 5, ends inside (the PnP form: every iteration available)", counts=_counts(100, i1=90), model_points=5, group=1, found=100,
         max_iters=100, expect=(1, 5, 90, 0)),
    dict(name="m = 5, a better one before the stop", counts=_counts(100, i1=80, i11=90), model_points=5, group=1, found=100, max_iters=100,
         expect=(11, 12, 90, 0)),
    dict(name="m = 5, a better one at the stop", counts=_counts(100, i1=80, i12=90), model_points=5, group=1, found=100, max_iters=100,
         expect=(1, 12, 80, 0)),
    dict(name="nothing found by the sampler", counts=_counts(96, i0=90), model_points=7, group=1, found=0, max_iters=1000, expect=(-1, 0, 0, 0)),
]
