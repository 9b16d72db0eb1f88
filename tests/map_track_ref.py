"""The rule of include/dvslam_hip.h "Tracking against the map" in plain Python / numpy, one landmark and one iteration at a time: what
csrc/map_track.hip must compute.  Stages 1-3 use Python floats (IEEE doubles) and ints in the header's order of operations, so every
integer output and every stage-1 double is comparable bit for bit; stage 4 calls math.sin / cos / sqrt and sums in index order, so it is
compared through its inlier flags and its cost.  search_brute is a second search with no grid at all; it must agree with search_grid.
refine() runs any schedule (first_round, n_rounds, n_iters) of the four rounds of ten steps, so that single Gauss-Newton steps can be
compared; gauss_newton_step can also sum in the header's lane order, and gauss_newton_step_ld restates the step in numpy.longdouble.
  STEP_MEASURED   the largest |difference| in any entry of the returned R or t between refine() with the longdouble step and refine() with
                  the float64 step — summing by index, and summing in the lane order — over STEP_SCHEDULES on step_scenes(); measured by
                  tests/test_map_track_cpu.py, which fails if it measures more than is recorded here.  The device is held to 10 x this."""
import math
import numpy as np

STEP_MEASURED = 2.5e-15         # measured 2.48e-15
STEP_SCHEDULES = [(0, 1, 1), (2, 1, 1), (0, 2, 1), (1, 2, 1), (0, 4, 10)]      # (first_round, n_rounds, n_iters)
MUTATIONS = ("w_one", "w_squared", "s2_one", "cross_half")

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
LM_RECORD = np.dtype([("u", "<f8"), ("v", "<f8"), ("visible", "<i4"), ("best_k", "<i4"), ("d_best", "<i4"), ("d_second", "<i4"),
                      ("proposed", "<i4"), ("kept", "<i4")])
OK, FEW_MATCHES, FEW_INLIERS, DEGENERATE = 0, 1, 2, 3


def default_sigma2(n_levels=8, factor=1.2):
    """the extractor's sigma2 table (csrc/orb.hip): scale kept in float, the factor a float widened, sigma2 a float product"""
    f = float(np.float32(factor))
    scale, out = np.float32(1.0), []
    for i in range(n_levels):
        if i > 0:
            scale = np.float32(float(scale) * f)
        out.append(float(np.float32(scale * scale)))
    return out


DEFAULTS = dict(min_z=0.05, max_z=20.0, radius=15.0, cell=32, max_hamming=50, ratio_pct=90, chi2_gate=5.991, min_matches=15, min_inliers=10,
                n_levels=8)


class Params:
    def __init__(self, rows, cols, fx, fy, cx, cy, **kw):
        self.rows, self.cols, self.fx, self.fy, self.cx, self.cy = int(rows), int(cols), float(fx), float(fy), float(cx), float(cy)
        for k, v in DEFAULTS.items():
            setattr(self, k, v)
        self.level_sigma2 = default_sigma2()
        for k, v in kw.items():
            if not hasattr(self, k):
                raise AttributeError(k)
            setattr(self, k, v)

    def with_(self, **kw):
        q = Params(self.rows, self.cols, self.fx, self.fy, self.cx, self.cy)
        q.__dict__.update(self.__dict__)
        q.__dict__.update(kw)
        return q


def pose_cw(R, t):
    """camera-to-world (R 3x3, t) -> (R_cw 9 floats row-major, t_cw 3 floats) in the header's arithmetic"""
    R = [float(v) for v in np.asarray(R, np.float64).reshape(9)]
    t = [float(v) for v in np.asarray(t, np.float64).reshape(3)]
    Rcw = [R[3 * j + i] for i in range(3) for j in range(3)]
    tcw = [-((R[i] * t[0] + R[3 + i] * t[1]) + R[6 + i] * t[2]) for i in range(3)]
    return Rcw, tcw


def pose_wc(Rcw, tcw):
    R = [Rcw[3 * j + i] for i in range(3) for j in range(3)]
    t = [-((Rcw[i] * tcw[0] + Rcw[3 + i] * tcw[1]) + Rcw[6 + i] * tcw[2]) for i in range(3)]
    return np.array(R).reshape(3, 3), np.array(t)


def camera_point(Rcw, tcw, X):
    return [((Rcw[3 * i] * X[0] + Rcw[3 * i + 1] * X[1]) + Rcw[3 * i + 2] * X[2]) + tcw[i] for i in range(3)]


def project_landmark(P, Rcw, tcw, xyz_row):
    """stage 1 for one landmark -> (visible, u, v); u = v = 0 when it is not visible"""
    X = [float(xyz_row[0]), float(xyz_row[1]), float(xyz_row[2])]   # float32 widened
    c = camera_point(Rcw, tcw, X)
    if not (P.min_z < c[2] and c[2] < P.max_z):
        return False, 0.0, 0.0
    u = P.fx * c[0] / c[2] + P.cx
    v = P.fy * c[1] / c[2] + P.cy
    if 0.0 <= u and u < float(P.cols) and 0.0 <= v and v < float(P.rows):
        return True, u, v
    return False, 0.0, 0.0


def binned(P, kp):
    x, y = np.float32(kp["x"]), np.float32(kp["y"])
    return bool(x >= np.float32(0) and x < np.float32(P.cols) and y >= np.float32(0) and y < np.float32(P.rows) and 0 <= int(kp["octave"]) < P.n_levels)


def bin_keypoints(P, kps):
    """-> (cell_start int32 [ncell + 1], order int32 [n_binned], n_unbinned): a counting sort, stable in keypoint index"""
    gw, gh = (P.cols + P.cell - 1) // P.cell, (P.rows + P.cell - 1) // P.cell
    cells = [[] for _ in range(gw * gh)]
    unb = 0
    for k in range(len(kps)):
        if not binned(P, kps[k]):
            unb += 1
            continue
        cells[(int(kps[k]["y"]) // P.cell) * gw + int(kps[k]["x"]) // P.cell].append(k)
    start = np.zeros(gw * gh + 1, np.int32)
    start[1:] = np.cumsum([len(c) for c in cells])
    order = np.array([k for c in cells for k in c], np.int32)
    return start, order, unb


def hamming(a, b):
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


def _pick(P, cand, ldesc_row, kdesc):
    """best = smallest (d, k); second = smallest d among the others -> (best_k, d_best, d_second, proposed)"""
    if not cand:
        return -1, -1, -1, 0
    keyed = sorted((hamming(ldesc_row, kdesc[k]), k) for k in cand)
    d_best, best_k = keyed[0]
    d_second = keyed[1][0] if len(keyed) > 1 else -1
    ok = d_best < P.max_hamming and (d_second < 0 or P.ratio_pct <= 0 or d_best * 100 < P.ratio_pct * d_second)
    return best_k, d_best, d_second, int(ok)


def _candidate(P, kp, u, v):
    return abs(float(kp["x"]) - u) <= P.radius and abs(float(kp["y"]) - v) <= P.radius


def search_grid(P, Rcw, tcw, xyz, ldesc, kps, kdesc):
    """stages 1-2, only the cells overlapping each window -> LM_RECORD array (kept still 0)"""
    start, order, _ = bin_keypoints(P, kps)
    gw, gh = (P.cols + P.cell - 1) // P.cell, (P.rows + P.cell - 1) // P.cell
    rec = np.zeros(len(xyz), LM_RECORD)
    rec["best_k"] = rec["d_best"] = rec["d_second"] = -1
    for j in range(len(xyz)):
        vis, u, v = project_landmark(P, Rcw, tcw, xyz[j])
        if not vis:
            continue
        xlo, xhi, ylo, yhi = u - P.radius, u + P.radius, v - P.radius, v + P.radius
        cx0 = 0 if xlo <= 0.0 else int(xlo) // P.cell
        cx1 = gw - 1 if xhi >= float(P.cols) else int(xhi) // P.cell
        cy0 = 0 if ylo <= 0.0 else int(ylo) // P.cell
        cy1 = gh - 1 if yhi >= float(P.rows) else int(yhi) // P.cell
        cand = []
        for cy in range(cy0, cy1 + 1):
            for cx in range(cx0, cx1 + 1):
                c = cy * gw + cx
                cand += [int(k) for k in order[start[c]:start[c + 1]] if _candidate(P, kps[k], u, v)]
        rec[j] = (u, v, 1) + _pick(P, cand, ldesc[j], kdesc) + (0,)
    return rec


def search_brute(P, Rcw, tcw, xyz, ldesc, kps, kdesc):
    """the same with no grid: every binned keypoint is tried for every visible landmark"""
    ok = [k for k in range(len(kps)) if binned(P, kps[k])]
    rec = np.zeros(len(xyz), LM_RECORD)
    rec["best_k"] = rec["d_best"] = rec["d_second"] = -1
    for j in range(len(xyz)):
        vis, u, v = project_landmark(P, Rcw, tcw, xyz[j])
        if vis:
            rec[j] = (u, v, 1) + _pick(P, [k for k in ok if _candidate(P, kps[k], u, v)], ldesc[j], kdesc) + (0,)
    return rec


def assign(rec, n_kp):
    """stage 3 -> (kp_lm int32, kp_dist int32); sets rec['kept']"""
    kp_lm = np.full(n_kp, -1, np.int32); kp_dist = np.full(n_kp, -1, np.int32)
    for j in range(len(rec)):                       # rows ascend: the first proposal at a distance is the lowest row
        if rec[j]["proposed"]:
            k, d = int(rec[j]["best_k"]), int(rec[j]["d_best"])
            if kp_lm[k] < 0 or d < kp_dist[k]:
                kp_lm[k], kp_dist[k] = j, d
    rec["kept"] = 0
    for k in range(n_kp):
        if kp_lm[k] >= 0:
            rec[kp_lm[k]]["kept"] = 1
    return kp_lm, kp_dist


# ---------------------------------------------------------------------------------------------------- stage 4
def chi_of(P, Rcw, tcw, X, px, octave):
    """-> (chi, c, ex, ey, s2); chi = inf where the point is not in front of the camera (c2 <= 0 or not finite: a position that is not
    finite gives no finite c2) or the octave has no sigma; such a pair has c = None"""
    if not 0 <= octave < P.n_levels:
        return math.inf, None, 0.0, 0.0, 1.0
    c = camera_point(Rcw, tcw, X)
    if not (c[2] > 0.0 and c[2] < math.inf):
        return math.inf, None, 0.0, 0.0, 1.0
    ex = px[0] - (P.fx * c[0] / c[2] + P.cx)
    ey = px[1] - (P.fy * c[1] / c[2] + P.cy)
    s2 = P.level_sigma2[octave]
    return (ex * ex + ey * ey) / s2, c, ex, ey, s2


def _exp_so3(w):
    th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
    th = math.sqrt(th2)
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if th < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + (math.sin(th) / th) * K + ((1.0 - math.cos(th)) / th2) * (K @ K)


def _add_in_lane_order(terms, shape):
    """the header's order: pair i on lane i mod 256 (a lane adds its pairs in ascending i, from 0.0), lane c + 8 k added in ascending k for
    each c < 8 (from 0.0), then the eight in order (from the first)"""
    lanes = np.zeros((256,) + shape)
    for i, v in terms:
        lanes[i % 256] += v
    eight = np.zeros((8,) + shape)
    for c in range(8):
        for k in range(32):
            eight[c] += lanes[c + 8 * k]
    tot = eight[0].copy()
    for c in range(1, 8):
        tot += eight[c]
    return tot


def gauss_newton_step(P, Rcw, tcw, X, px, octs, inl, robust, sums="index", mutate=None):
    """one iteration -> (R_cw, t_cw) updated, or None (a pivot too small / something not finite).  A flagged pair in front of the camera
    whose residual is not finite (a pixel that is not finite) ends the refinement.  sums: "index" adds the pairs in index order, "lanes"
    in the header's lane order.  mutate: one of MUTATIONS, a deliberately WRONG step, for the tests that show a comparison has teeth"""
    assert sums in ("index", "lanes") and (mutate is None or mutate in MUTATIONS)
    Hs, bs = [], []
    for i in range(len(X)):
        if not inl[i]:
            continue
        chi, c, ex, ey, s2 = chi_of(P, Rcw, tcw, X[i], px[i], int(octs[i]))
        if c is None:
            continue
        if not math.isfinite(chi):
            return None
        w = math.sqrt(P.chi2_gate / chi) if (robust and chi > P.chi2_gate) else 1.0
        if mutate == "w_one":
            w = 1.0
        if mutate == "w_squared" and robust and chi > P.chi2_gate:
            w = P.chi2_gate / chi
        if mutate == "s2_one":
            s2 = 1.0
        iz = 1.0 / c[2]
        a, bb = P.fx * iz, P.fy * iz
        a2, b2 = -(a * c[0]) * iz, -(bb * c[1]) * iz
        Ju = np.array([a2 * c[1], a * c[2] - a2 * c[0], -(a * c[1]), a, 0.0, a2])
        Jv = np.array([b2 * c[1] - bb * c[2], -(b2 * c[0]), bb * c[0], 0.0, bb, b2])
        Hi = np.outer(Ju, Ju) + np.outer(Jv, Jv)
        if mutate == "cross_half":
            Hi[0, 4] *= 0.5; Hi[4, 0] *= 0.5
        Hs.append((i, (w / s2) * Hi))
        bs.append((i, (w / s2) * (Ju * ex + Jv * ey)))
    if sums == "lanes":
        H, b = _add_in_lane_order(Hs, (6, 6)), _add_in_lane_order(bs, (6,))
    else:
        H = np.zeros((6, 6)); b = np.zeros(6)
        for (_, h), (_, g) in zip(Hs, bs):
            H += h
            b += g
    if not np.isfinite(H).all():
        return None
    maxd = max(0.0, float(np.diag(H).max()))
    L = np.zeros((6, 6))
    for j in range(6):
        p = H[j, j] - float(L[j, :j] @ L[j, :j])
        if not math.isfinite(p) or p <= 1e-10 * maxd:
            return None
        L[j, j] = math.sqrt(p)
        for i in range(j + 1, 6):
            L[i, j] = (H[i, j] - float(L[i, :j] @ L[j, :j])) / L[j, j]
    y = np.zeros(6); d = np.zeros(6)
    for i in range(6):
        y[i] = (b[i] - float(L[i, :i] @ y[:i])) / L[i, i]
    for i in range(5, -1, -1):
        d[i] = (y[i] - float(L[i + 1:, i] @ d[i + 1:])) / L[i, i]
    if not np.isfinite(d).all():
        return None
    E = _exp_so3(d[:3])
    Rn = E @ np.array(Rcw).reshape(3, 3)
    tn = E @ np.array(tcw) + d[3:]
    if not (np.isfinite(Rn).all() and np.isfinite(tn).all()):
        return None
    return [float(v) for v in Rn.reshape(9)], [float(v) for v in tn]


def gauss_newton_step_ld(P, Rcw, tcw, X, px, octs, inl, robust):
    """the same iteration restated in numpy.longdouble from the inputs to the new pose — residual, weight, Jacobian, sums in index order,
    Cholesky, Rodrigues — and rounded to float64 once at the end: the yardstick of STEP_MEASURED.  No pivot test: for well-posed scenes"""
    f = np.longdouble
    R = np.array(Rcw, f).reshape(3, 3); t = np.array(tcw, f)
    fx, fy, cx, cy, gate = f(P.fx), f(P.fy), f(P.cx), f(P.cy), f(P.chi2_gate)
    H = np.zeros((6, 6), f); b = np.zeros(6, f); z = f(0)
    for i in range(len(X)):
        o = int(octs[i])
        if not inl[i] or not 0 <= o < P.n_levels:
            continue
        c = R @ np.array(X[i], f) + t
        if not (c[2] > 0 and np.isfinite(c[2])):
            continue
        e = np.array([f(px[i][0]) - (fx * c[0] / c[2] + cx), f(px[i][1]) - (fy * c[1] / c[2] + cy)])
        s2 = f(P.level_sigma2[o])
        chi = (e @ e) / s2
        w = np.sqrt(gate / chi) if (robust and chi > gate) else f(1)
        Jp = np.array([[fx / c[2], z, -fx * c[0] / (c[2] * c[2])], [z, fy / c[2], -fy * c[1] / (c[2] * c[2])]])      # d(u, v) / dc
        Jc = np.array([[z, c[2], -c[1], f(1), z, z], [-c[2], z, c[0], z, f(1), z], [c[1], -c[0], z, z, z, f(1)]])    # dc / d(omega, upsilon) = [-[c]x | I]
        J = Jp @ Jc
        H += (w / s2) * (J.T @ J)
        b += (w / s2) * (J.T @ e)
    L = np.zeros((6, 6), f)
    for j in range(6):
        L[j, j] = np.sqrt(H[j, j] - L[j, :j] @ L[j, :j])
        for i in range(j + 1, 6):
            L[i, j] = (H[i, j] - L[i, :j] @ L[j, :j]) / L[j, j]
    y = np.zeros(6, f); d = np.zeros(6, f)
    for i in range(6):
        y[i] = (b[i] - L[i, :i] @ y[:i]) / L[i, i]
    for i in range(5, -1, -1):
        d[i] = (y[i] - L[i + 1:, i] @ d[i + 1:]) / L[i, i]
    w3 = d[:3]
    th2 = w3 @ w3; th = np.sqrt(th2)
    K = np.array([[z, -w3[2], w3[1]], [w3[2], z, -w3[0]], [-w3[1], w3[0], z]])
    E = np.eye(3, dtype=f) + (np.sin(th) / th) * K + ((1 - np.cos(th)) / th2) * (K @ K)
    Rn = E @ R; tn = E @ t + d[3:]
    if not (np.isfinite(Rn.astype(np.float64)).all() and np.isfinite(tn.astype(np.float64)).all()):
        return None
    return [float(v) for v in Rn.reshape(9)], [float(v) for v in tn]


def refine(P, R, t, X, px, octs, first_round=0, n_rounds=4, n_iters=10, step=gauss_newton_step):
    """stage 4 on explicit correspondences -> dict(status, R, t, cost, n_inliers, inlier uint8 [n], chi_rounds [n_rounds][n] — the chi
    values of the classification after each round that ran).  The product runs rounds 0 .. 3 of ten steps; any other schedule runs rounds
    first_round .. first_round + n_rounds - 1 of n_iters steps (round r is robust iff r < 2; every pair counts as an inlier before the
    first round that runs), for comparing single steps.  step: the iteration, gauss_newton_step's signature"""
    assert 0 <= first_round and 1 <= n_rounds and first_round + n_rounds <= 4 and 1 <= n_iters <= 10
    X = np.asarray(X, np.float64).reshape(-1, 3); px = np.asarray(px, np.float64).reshape(-1, 2); octs = np.asarray(octs).reshape(-1)
    n = len(X)
    R0, t0 = np.array(R, np.float64).reshape(3, 3).copy(), np.array(t, np.float64).reshape(3).copy()
    out = dict(status=OK, R=R0, t=t0, cost=0.0, n_inliers=0, inlier=np.zeros(n, np.uint8), chi_rounds=[], n_matches=n)
    if n < P.min_matches:
        out["status"] = FEW_MATCHES
        return out
    Rcw, tcw = pose_cw(R0, t0)
    Xl, pl = [[float(v) for v in r] for r in X], [[float(v) for v in r] for r in px]
    inl = np.ones(n, np.uint8)
    cost = 0.0
    for rnd in range(first_round, first_round + n_rounds):
        for _ in range(n_iters):
            new = step(P, Rcw, tcw, Xl, pl, octs, inl, rnd < 2)
            if new is None:
                out["status"] = DEGENERATE
                return out
            Rcw, tcw = new
        chis = np.array([chi_of(P, Rcw, tcw, Xl[i], pl[i], int(octs[i]))[0] for i in range(n)])
        out["chi_rounds"].append(chis)
        inl = (chis <= P.chi2_gate).astype(np.uint8)
        cost = float(chis[inl != 0].sum())
        if not math.isfinite(cost):
            out["status"] = DEGENERATE
            return out
    out.update(cost=cost, n_inliers=int(inl.sum()), inlier=inl, Rcw=Rcw, tcw=tcw)
    if int(inl.sum()) < P.min_inliers:
        out["status"] = FEW_INLIERS
        return out
    out["R"], out["t"] = pose_wc(Rcw, tcw)
    return out


def track(P, R, t, xyz, ldesc, kps, kdesc, search=search_grid):
    """stages 1-4 -> dict: rec, kp_lm, kp_dist, kp_inlier, counts and refine()'s outputs"""
    Rcw, tcw = pose_cw(R, t)
    rec = search(P, Rcw, tcw, xyz, ldesc, kps, kdesc)
    kp_lm, kp_dist = assign(rec, len(kps))
    ks = [k for k in range(len(kps)) if kp_lm[k] >= 0]
    X = np.array([[float(v) for v in xyz[kp_lm[k]]] for k in ks], np.float64).reshape(-1, 3)
    px = np.array([[float(kps[k]["x"]), float(kps[k]["y"])] for k in ks], np.float64).reshape(-1, 2)
    octs = np.array([int(kps[k]["octave"]) for k in ks], np.int32)
    out = refine(P, R, t, X, px, octs)
    kp_inl = np.zeros(len(kps), np.uint8)
    if out["status"] in (OK, FEW_INLIERS):
        kp_inl[ks] = out["inlier"]
    out.update(rec=rec, kp_lm=kp_lm, kp_dist=kp_dist, kp_inlier=kp_inl, n_visible=int(rec["visible"].sum()), n_proposed=int(rec["proposed"].sum()),
               n_unbinned=bin_keypoints(P, kps)[2])
    return out


def gate_margin(P, res):
    """the smallest relative distance of any chi to the gate over the classifications that ran"""
    m = math.inf
    for chis in res["chi_rounds"]:
        f = chis[np.isfinite(chis)]
        if len(f):
            m = min(m, float(np.abs(f - P.chi2_gate).min()) / P.chi2_gate)
    return m


def scipy_optimum(P, Rcw, tcw, X, px, octs, inl):
    """the least-squares optimum of sum chi over the pairs flagged in `inl`, from (R_cw, t_cw), by scipy.optimize.least_squares"""
    from scipy.optimize import least_squares
    idx = np.flatnonzero(inl)
    Xs = np.asarray(X, np.float64).reshape(-1, 3)[idx]; ps = np.asarray(px, np.float64).reshape(-1, 2)[idx]
    sig = np.sqrt(np.array([P.level_sigma2[int(o)] for o in np.asarray(octs)[idx]]))
    R0, t0 = np.array(Rcw).reshape(3, 3), np.array(tcw)

    def fun(d):
        E = _exp_so3(d[:3])
        c = Xs @ (E @ R0).T + (E @ t0 + d[3:])
        u = P.fx * c[:, 0] / c[:, 2] + P.cx; v = P.fy * c[:, 1] / c[:, 2] + P.cy
        return np.concatenate([(ps[:, 0] - u) / sig, (ps[:, 1] - v) / sig])
    sol = least_squares(fun, np.zeros(6), method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15)
    return float((sol.fun ** 2).sum())


# ---------------------------------------------------------------------------------------------------- scenes
def rot(axis, deg):
    a = math.radians(deg); c, s = math.cos(a), math.sin(a)
    return {"x": np.array([[1, 0, 0], [0, c, -s], [0, s, c]]), "y": np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]),
            "z": np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])}[axis]


def refine_scene(n=300, outliers=0.15, seed=7, noise=0.6, gross_spread=None):
    """explicit correspondences: n landmarks seen from a known pose with pixel noise noise * sqrt(sigma2) and a share of gross outliers;
    (anywhere in the image, or displaced by up to gross_spread pixels); the prior is 3.7 degrees and 7 cm off -> dict(P, R_true, t_true, R0, t0, X, px, oct, gross)"""
    rng = np.random.default_rng(seed)
    P = Params(480, 640, 520.0, 515.0, 318.5, 241.25)
    R_true = rot("y", 12.0) @ rot("x", -5.0); t_true = np.array([0.3, -0.1, 0.2])
    Rcw, tcw = R_true.T, -R_true.T @ t_true
    c = np.stack([rng.uniform(-2.2, 2.2, n), rng.uniform(-1.6, 1.6, n), rng.uniform(2.5, 8.0, n)], 1)
    octs = rng.integers(0, P.n_levels, n).astype(np.int32)
    px = np.stack([P.fx * c[:, 0] / c[:, 2] + P.cx, P.fy * c[:, 1] / c[:, 2] + P.cy], 1)
    px += rng.normal(0, noise, (n, 2)) * np.sqrt(np.array(P.level_sigma2)[octs])[:, None]
    gross = rng.random(n) < outliers
    if gross_spread is None:                 # anywhere in the image
        px[gross] = np.stack([rng.uniform(0, P.cols, gross.sum()), rng.uniform(0, P.rows, gross.sum())], 1)
    else:                                    # displaced by up to gross_spread pixels each way: still far outside the gate, but a few land inside it
        px[gross] += rng.uniform(-gross_spread, gross_spread, (int(gross.sum()), 2))
    X = (c - tcw) @ Rcw                      # X_w = R (c - t_cw)
    axis = np.array([0.5, -0.7, 0.5]); axis /= np.linalg.norm(axis)
    dR = _exp_so3(list(axis * math.radians(3.7)))
    dt = np.array([0.04, -0.05, 0.028]); dt *= 0.07 / np.linalg.norm(dt)
    return dict(P=P, R_true=R_true, t_true=t_true, R0=R_true @ dR, t0=t_true + dt, X=np.ascontiguousarray(X), px=np.ascontiguousarray(px), oct=octs,
                gross=gross)


def step_scenes():
    """the scenes the single steps are compared on: the prior is 3.7 degrees and 7 cm off, so the first step is large"""
    return [refine_scene(), refine_scene(n=257)]


def outlier_scene():
    """gross outliers only: every pixel is displaced by up to 25 px each way (the gate is 2.45 sigma, 2.4 .. 8.8 px); a handful fall inside the
    gate of whatever pose the rounds settle on, fewer than min_inliers"""
    return refine_scene(n=120, outliers=1.0, seed=1, gross_spread=25.0)


def track_scene(n=300, outliers=0.15, seed=9, noise=0.6, prior_deg=0.5, prior_m=0.01):
    """a whole frame for stages 1-4: refine_scene's geometry with float landmarks, a keypoint at every (noisy) projection carrying its
    landmark's descriptor with a few bits flipped, gross outliers displaced by 8 .. 12 px (inside the search window, outside the gate), and
    a prior close enough for the window -> dict(P, R0, t0, R_true, t_true, xyz, ldesc, ids, kps, kdesc)"""
    rng = np.random.default_rng(seed)
    s = refine_scene(n, 0.0, seed, noise)
    P = s["P"]
    px = s["px"].copy()
    gross = rng.random(n) < outliers
    ang = rng.uniform(0, 2 * math.pi, n); rad = rng.uniform(8.0, 12.0, n)
    px[gross] += np.stack([rad * np.cos(ang), rad * np.sin(ang)], 1)[gross]
    inside = (px[:, 0] >= 0) & (px[:, 0] < P.cols - 1) & (px[:, 1] >= 0) & (px[:, 1] < P.rows - 1)
    ldesc = random_descriptors(rng, n)
    kdesc = ldesc.copy()
    for k in range(n):
        for b in rng.choice(256, int(rng.integers(0, 9)), replace=False):
            kdesc[k, b >> 3] ^= np.uint8(1 << (b & 7))
    perm = rng.permutation(np.flatnonzero(inside))               # keypoint order is not landmark order
    kps = keypoints(px[perm].astype(np.float32))
    kps["octave"] = s["oct"][perm]
    axis = np.array([-0.3, 0.8, 0.5]); axis /= np.linalg.norm(axis)
    dt = np.array([0.5, 0.5, -0.7]); dt *= prior_m / np.linalg.norm(dt)
    return dict(P=P, R_true=s["R_true"], t_true=s["t_true"], R0=s["R_true"] @ _exp_so3(list(axis * math.radians(prior_deg))), t0=s["t_true"] + dt,
                xyz=s["X"].astype(np.float32), ldesc=ldesc, ids=np.arange(n, dtype=np.int64) * 3 + 100, kps=kps, kdesc=np.ascontiguousarray(kdesc[perm]),
                gross=gross)


def random_descriptors(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def keypoints(xy, octave=0):
    k = np.zeros(len(xy), KP_DTYPE)
    if len(xy):
        xy = np.asarray(xy, np.float32).reshape(-1, 2)
        k["x"], k["y"] = xy[:, 0], xy[:, 1]
    k["size"], k["angle"], k["response"], k["octave"], k["class_id"] = 31.0, 0.0, 50.0, octave, -1
    return k


def search_scene(P, n_lm, n_kp, seed, R=None, t=None, flip_bits=12, depth=(1.0, 3.0), jitter=4.0, group=5, kp_stride=1):
    """landmarks spread over (and a little beyond) the view of pose (R, t); keypoint k sits near the projection of landmark
    (k * kp_stride) % n_lm with that landmark's descriptor and a few bits flipped, so windows overlap and landmarks compete.  The landmarks
    come in groups of `group`: with the default, the last of every five nearly repeats the one before it; with group < 0 every landmark but
    the first of each -group nearly repeats the one before it, so a keypoint on a group's first landmark (kp_stride = -group) is what the
    whole group proposes to -> (xyz f32, ldesc, kps, kdesc)"""
    rng = np.random.default_rng(seed)
    R = np.eye(3) if R is None else np.asarray(R, np.float64); t = np.zeros(3) if t is None else np.asarray(t, np.float64)
    u = rng.uniform(-0.1 * P.cols, 1.1 * P.cols, n_lm); v = rng.uniform(-0.1 * P.rows, 1.1 * P.rows, n_lm); z = rng.uniform(depth[0], depth[1], n_lm)
    ldesc = random_descriptors(rng, n_lm)
    copies = range(group - 1, n_lm, group) if group > 0 else [j for j in range(n_lm) if j % -group]
    for j in copies:                              # a landmark that nearly repeats the one before it: they compete for a keypoint
        u[j], v[j], z[j] = u[j - 1] + rng.uniform(-2, 2), v[j - 1] + rng.uniform(-2, 2), z[j - 1]
        ldesc[j] = ldesc[j - 1]
        ldesc[j, int(rng.integers(0, 32))] ^= np.uint8(1 << int(rng.integers(0, 8)))
    c = np.stack([(u - P.cx) * z / P.fx, (v - P.cy) * z / P.fy, z], 1)
    xyz = (c @ R.T + t).astype(np.float32)
    xy = np.zeros((n_kp, 2), np.float32); kdesc = random_descriptors(rng, n_kp)
    for k in range(n_kp):
        if n_lm:
            j = (k * kp_stride) % n_lm
            xy[k] = (u[j] + rng.uniform(-jitter, jitter), v[j] + rng.uniform(-jitter, jitter))
            d = ldesc[j].copy()
            for b in rng.choice(256, int(rng.integers(0, flip_bits + 1)), replace=False):
                d[b >> 3] ^= np.uint8(1 << (b & 7))
            kdesc[k] = d
        else:
            xy[k] = (rng.uniform(0, P.cols), rng.uniform(0, P.rows))
    xy[:, 0] = np.clip(xy[:, 0], 0, np.float32(P.cols) - np.float32(0.01)); xy[:, 1] = np.clip(xy[:, 1], 0, np.float32(P.rows) - np.float32(0.01))
    kps = keypoints(xy)
    kps["octave"] = rng.integers(0, P.n_levels, n_kp)
    return xyz, ldesc, kps, kdesc


# ---------------------------------------------------------------------------------------------------- scenes at frame structure
FRAME_R, FRAME_T = rot("y", 3.0) @ rot("x", -2.0), np.array([0.05, -0.02, 0.1])


def frame_params(**kw):
    """640 x 480 with refine_scene's intrinsics: 300 cells of 32 pixels, 1200 of 16"""
    return Params(480, 640, 520.0, 515.0, 318.5, 241.25, **kw)


def small_params(**kw):
    """100 x 70, not a multiple of the 32-pixel cell, with z gates that are exact floats (a 4 x 3 grid)"""
    return Params(70, 100, 80.0, 80.0, 50.0, 35.0, **dict(dict(min_z=0.5, max_z=4.0), **kw))


def sparse_ids(n, seed):
    """ascending ids that are not row numbers"""
    return np.cumsum(np.random.default_rng(seed).integers(1, 9, n)).astype(np.int64) + (1 << 40)


def frame_scene(P, n_lm, n_kp):
    """search_scene seen from (FRAME_R, FRAME_T) with seed 20 + n_kp -> (xyz, ldesc, kps, kdesc, ids)"""
    return search_scene(P, n_lm, n_kp, 20 + n_kp, FRAME_R, FRAME_T) + (sparse_ids(n_lm, n_lm),)


def crowded_scene(P, n_lm=20000, n_kp=2000, seed=77):
    """many workgroups of landmarks on few keypoints: groups of ten near-copies, one keypoint on the first of each group, so a matched
    keypoint has up to ten proposals to choose from -> (xyz, ldesc, kps, kdesc, ids)"""
    return search_scene(P, n_lm, n_kp, seed, FRAME_R, FRAME_T, group=-10, kp_stride=10) + (sparse_ids(n_lm, seed),)


def proposals_per_keypoint(rec, n_kp):
    return np.bincount(rec["best_k"][rec["proposed"] == 1], minlength=n_kp)


def dense_cell_scene(P, n_before, seed=1, n_dense=300, n_lm=65):
    """n_dense keypoints in cell (1, 1) of small_params()' grid — more than one workgroup's worth in ONE cell — and n_lm landmarks around
    them, identity pose.  n_before > 0: that many keypoints in the lower-numbered cells (y < 32), so the dense cell's CSR segment starts
    at slot n_before; n_before == 0: 60 keypoints in the two cells to its right instead.  The keypoint indices of the dense cell and of
    the others interleave, so the CSR order is not the index order -> (xyz, ldesc, kps, kdesc, dense cell index)"""
    assert P.cell == 32 and P.cols == 100 and P.rows == 70
    rng = np.random.default_rng(seed)
    n_other = n_before if n_before else 60
    n_kp = n_dense + n_other
    other = np.zeros(n_kp, bool)
    other[np.round(np.linspace(0, n_kp - 1, n_other)).astype(int)] = True          # spread evenly through the indices
    assert other.sum() == n_other
    xy = np.zeros((n_kp, 2), np.float32)
    xy[~other] = 32 + rng.uniform(0, 31.9, (n_dense, 2))
    if n_before:
        xy[other] = np.stack([rng.uniform(0, 99.9, n_other), rng.uniform(0, 31.9, n_other)], 1)
    else:
        xy[other] = np.stack([rng.uniform(64, 99.9, n_other), rng.uniform(32, 63.9, n_other)], 1)
    ldesc = random_descriptors(rng, n_lm)
    kdesc = np.zeros((n_kp, 32), np.uint8)
    for k in range(n_kp):                                                           # keypoint k carries landmark k % n_lm's descriptor, a few bits flipped
        d = ldesc[k % n_lm].copy()
        for b in rng.choice(256, int(rng.integers(0, 13)), replace=False):
            d[b >> 3] ^= np.uint8(1 << (b & 7))
        kdesc[k] = d
    z = rng.uniform(1.0, 3.0, n_lm)
    xyz = np.zeros((n_lm, 3), np.float32)
    dense = np.flatnonzero(~other)
    for j in range(n_lm):                                                           # landmark j next to the first dense keypoint that carries its descriptor
        k = dense[dense % n_lm == j][0]
        xyz[j] = ((xy[k, 0] + 1.5 - P.cx) * z[j] / P.fx, (xy[k, 1] - 1.0 - P.cy) * z[j] / P.fy, z[j])
    kps = keypoints(xy)
    kps["octave"] = rng.integers(0, P.n_levels, n_kp)
    return xyz, ldesc, kps, kdesc, 1 * 4 + 1


# ---------------------------------------------------------------------------------------------------- scenes for the stated pair rules
def _world(s, c):
    """the world point that the scene's TRUE pose sees at camera point c"""
    Rcw, tcw = s["R_true"].T, -s["R_true"].T @ s["t_true"]
    return (np.asarray(c, np.float64) - tcw) @ Rcw


def pair_rule_scene():
    """refine_scene() with 8 points moved behind the true camera (c2 in -4 .. -0.5) and 8 others given octave -1 or n_levels: 16 pairs
    that add nothing to any sum -> (scene, behind rows, bad-octave rows)"""
    s = refine_scene()
    rng = np.random.default_rng(3)
    behind, badoct = np.arange(5, 300, 37), np.arange(11, 300, 41)[:8]
    assert len(behind) == 8 and len(badoct) == 8 and not set(behind) & set(badoct)
    X, oc = s["X"].copy(), s["oct"].copy()
    for i in behind:
        X[i] = _world(s, [rng.uniform(-1, 1), rng.uniform(-1, 1), -rng.uniform(0.5, 4.0)])
    oc[badoct[::2]] = -1; oc[badoct[1::2]] = s["P"].n_levels
    return dict(s, X=np.ascontiguousarray(X), oct=oc), behind, badoct


def crossing_scene():
    """refine_scene() with point 7 at camera depth 0.02 m under the true pose: behind the camera at the prior, so the first step skips it,
    in front of it and an inlier at the end -> (scene, 7)"""
    s = refine_scene()
    X = s["X"].copy()
    X[7] = _world(s, [0.01, 0.01, 0.02])
    px = s["px"].copy()
    return dict(s, X=np.ascontiguousarray(X), px=px), 7
