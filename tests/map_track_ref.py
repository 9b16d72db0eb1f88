"""The rule of include/dvslam_hip.h "Tracking against the map" in plain Python / numpy, one landmark and one iteration at a time: what
csrc/map_track.hip must compute.  Stages 1-3 use Python floats (IEEE doubles) and ints in the header's order of operations, so every
integer output and every stage-1 double is comparable bit for bit; stage 4 calls math.sin / cos / sqrt and sums in index order, so it is
compared through its inlier flags and its cost.  search_brute is a second search with no grid at all; it must agree with search_grid."""
import math
import numpy as np

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
    """-> (chi, c, ex, ey, s2); chi = inf where the point is not in front of the camera or the octave has no sigma"""
    if not 0 <= octave < P.n_levels:
        return math.inf, None, 0.0, 0.0, 1.0
    c = camera_point(Rcw, tcw, X)
    if not c[2] > 0.0:
        return math.inf, c, 0.0, 0.0, 1.0
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


def gauss_newton_step(P, Rcw, tcw, X, px, octs, inl, robust):
    """one iteration -> (R_cw, t_cw) updated, or None (a pivot too small / something not finite)"""
    H = np.zeros((6, 6)); b = np.zeros(6)
    for i in range(len(X)):
        if not inl[i]:
            continue
        chi, c, ex, ey, s2 = chi_of(P, Rcw, tcw, X[i], px[i], int(octs[i]))
        if not math.isfinite(chi):
            continue
        w = math.sqrt(P.chi2_gate / chi) if (robust and chi > P.chi2_gate) else 1.0
        iz = 1.0 / c[2]
        a, bb = P.fx * iz, P.fy * iz
        a2, b2 = -(a * c[0]) * iz, -(bb * c[1]) * iz
        Ju = np.array([a2 * c[1], a * c[2] - a2 * c[0], -(a * c[1]), a, 0.0, a2])
        Jv = np.array([b2 * c[1] - bb * c[2], -(b2 * c[0]), bb * c[0], 0.0, bb, b2])
        H += (w / s2) * (np.outer(Ju, Ju) + np.outer(Jv, Jv))
        b += (w / s2) * (Ju * ex + Jv * ey)
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


def refine(P, R, t, X, px, octs):
    """stage 4 on explicit correspondences -> dict(status, R, t, cost, n_inliers, inlier uint8 [n], chi_rounds [4][n] — the chi values of
    the classification after each round that ran)"""
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
    for rnd in range(4):
        for _ in range(10):
            step = gauss_newton_step(P, Rcw, tcw, Xl, pl, octs, inl, rnd < 2)
            if step is None:
                out["status"] = DEGENERATE
                return out
            Rcw, tcw = step
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


def search_scene(P, n_lm, n_kp, seed, R=None, t=None, flip_bits=12, depth=(1.0, 3.0), jitter=4.0):
    """landmarks spread over (and a little beyond) the view of pose (R, t); keypoint k sits near the projection of landmark k % n_lm with
    that landmark's descriptor and a few bits flipped, so windows overlap and landmarks compete -> (xyz f32, ldesc, kps, kdesc)"""
    rng = np.random.default_rng(seed)
    R = np.eye(3) if R is None else np.asarray(R, np.float64); t = np.zeros(3) if t is None else np.asarray(t, np.float64)
    u = rng.uniform(-0.1 * P.cols, 1.1 * P.cols, n_lm); v = rng.uniform(-0.1 * P.rows, 1.1 * P.rows, n_lm); z = rng.uniform(depth[0], depth[1], n_lm)
    ldesc = random_descriptors(rng, n_lm)
    for j in range(4, n_lm, 5):                   # every fifth landmark nearly repeats the one before it: the two compete for a keypoint
        u[j], v[j], z[j] = u[j - 1] + rng.uniform(-2, 2), v[j - 1] + rng.uniform(-2, 2), z[j - 1]
        ldesc[j] = ldesc[j - 1]
        ldesc[j, int(rng.integers(0, 32))] ^= np.uint8(1 << int(rng.integers(0, 8)))
    c = np.stack([(u - P.cx) * z / P.fx, (v - P.cy) * z / P.fy, z], 1)
    xyz = (c @ R.T + t).astype(np.float32)
    xy = np.zeros((n_kp, 2), np.float32); kdesc = random_descriptors(rng, n_kp)
    for k in range(n_kp):
        if n_lm:
            j = k % n_lm
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
