"""LandmarkInfo::triangulate (backend.cpp:439-613) restated in float64 numpy, operation for operation as csrc/triangulate.hip runs it
(the issue's steps 1-8): every sum in the reference's order, no fused operations, float32 where the reference rounds to float.  The
arithmetic is elementwise over landmarks that have the same number of views, so each landmark sees exactly the scalar sequence of
operations (numpy float64 / float32 operations are IEEE, correctly rounded).  The same two departures as the kernel: gamma =
sqrt(p * p + beta * beta) in place of hypot, and the gate's atan2 is numpy's (scenes stay clear of the 5 degree bound).

Pose convention: x_cam = R X + t (P = K [R | t], C = -R^T t), R row-major 3 x 3 per keyframe."""
import numpy as np

UPDATED, FEW_VIEWS, LOW_PARALLAX, DEGENERATE, REPROJECTION, DEPTH = range(6)
MIN_PARALLAX = 0.0175 * 5
EPS = 10.0 * np.finfo(np.float64).eps


def _cams(R, t, kf, fx, fy, cx, cy):
    """P (..., 3, 4) and C (..., 3) of keyframes kf"""
    r = R[kf]; tt = t[kf]
    P = np.zeros(kf.shape + (3, 4))
    for k in range(3):
        P[..., 0, k] = fx * r[..., k] + cx * r[..., 6 + k]
        P[..., 1, k] = fy * r[..., 3 + k] + cy * r[..., 6 + k]
        P[..., 2, k] = r[..., 6 + k]
    P[..., 0, 3] = fx * tt[..., 0] + cx * tt[..., 2]
    P[..., 1, 3] = fy * tt[..., 1] + cy * tt[..., 2]
    P[..., 2, 3] = tt[..., 2]
    C = np.zeros(kf.shape + (3,))
    for k in range(3):
        C[..., k] = -(r[..., k] * tt[..., 0] + r[..., 3 + k] * tt[..., 1] + r[..., 6 + k] * tt[..., 2])
    return P, C


def _norm3(a):
    return np.sqrt(a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1] + a[..., 2] * a[..., 2])


def jacobi_null_vectors(At):
    """OpenCV 4.x JacobiSVDImpl_<double> on At (n landmarks x 4 rows x m) -> (sorted Vt's row 3 (n, 4), sweeps run (n,))"""
    At = At.copy()
    n, _, m = At.shape
    max_iter = max(m, 30)
    W = np.zeros((n, 4))
    for i in range(4):
        sd = np.zeros(n)
        for k in range(m):
            sd = sd + At[:, i, k] * At[:, i, k]
        W[:, i] = sd
    Vt = np.tile(np.eye(4), (n, 1, 1))
    active = np.ones(n, bool)
    sweeps = np.zeros(n, np.int64)
    with np.errstate(all="ignore"):
        for _ in range(max_iter):
            if not active.any():
                break
            sweeps += active
            changed = np.zeros(n, bool)
            for i in range(3):
                for j in range(i + 1, 4):
                    a = W[:, i]; b = W[:, j]
                    p = np.zeros(n)
                    for k in range(m):
                        p = p + At[:, i, k] * At[:, j, k]
                    rot = active & ~(np.abs(p) <= EPS * np.sqrt(a * b))
                    if not rot.any():
                        continue
                    p = p * 2
                    beta = a - b
                    gamma = np.sqrt(p * p + beta * beta)
                    neg = beta < 0
                    s_n = np.sqrt(((gamma - beta) * 0.5) / gamma)
                    c_n = p / (gamma * s_n * 2)
                    c_p = np.sqrt((gamma + beta) / (gamma * 2))
                    s_p = p / (gamma * c_p * 2)
                    c = np.where(neg, c_n, c_p); s = np.where(neg, s_n, s_p)
                    na = np.zeros(n); nb = np.zeros(n)
                    for k in range(m):
                        ai = At[:, i, k]; aj = At[:, j, k]
                        t0 = c * ai + s * aj
                        t1 = -s * ai + c * aj
                        At[:, i, k] = np.where(rot, t0, ai); At[:, j, k] = np.where(rot, t1, aj)
                        na = na + t0 * t0; nb = nb + t1 * t1
                    W[:, i] = np.where(rot, na, a); W[:, j] = np.where(rot, nb, b)
                    vi = Vt[:, i, :].copy(); vj = Vt[:, j, :].copy()
                    Vt[:, i, :] = np.where(rot[:, None], c[:, None] * vi + s[:, None] * vj, vi)
                    Vt[:, j, :] = np.where(rot[:, None], -s[:, None] * vi + c[:, None] * vj, vj)
                    changed |= rot
            active &= changed
    for i in range(4):
        sd = np.zeros(n)
        for k in range(m):
            sd = sd + At[:, i, k] * At[:, i, k]
        W[:, i] = np.sqrt(sd)
    idx = np.tile(np.arange(4), (n, 1))
    rows = np.arange(n)
    for i in range(3):
        j = np.full(n, i)
        for k in range(i + 1, 4):
            j = np.where(W[rows, j] < W[:, k], k, j)
        wi = W[:, i].copy(); W[:, i] = W[rows, j]; W[rows, j] = wi
        ii = idx[:, i].copy(); idx[:, i] = idx[rows, j]; idx[rows, j] = ii
    return Vt[rows, idx[:, 3], :], sweeps


def _valid_views(offsets, view_kf):
    return [np.nonzero(view_kf[offsets[l]:offsets[l + 1]] >= 0)[0] + offsets[l] for l in range(len(offsets) - 1)]


def triangulate(R, t, fx, fy, cx, cy, offsets, view_kf, view_px, xyz, details=False):
    """-> (positions float32 (nlm, 3), status int32 (nlm,)); details=True adds a dict with the null vectors, sweeps and max parallax"""
    R = np.asarray(R, np.float64).reshape(-1, 9); t = np.asarray(t, np.float64).reshape(-1, 3)
    offsets = np.asarray(offsets, np.int64); view_kf = np.asarray(view_kf, np.int32)
    view_px = np.asarray(view_px, np.float32).reshape(-1, 2); xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    fx, fy, cx, cy = float(fx), float(fy), float(cx), float(cy)
    nlm = len(offsets) - 1
    out = xyz.copy(); status = np.full(nlm, UPDATED, np.int32)
    info = dict(x=np.full((nlm, 4), np.nan), sweeps=np.zeros(nlm, np.int64), max_angle=np.zeros(nlm))
    views = _valid_views(offsets, view_kf)
    V = np.array([len(v) for v in views], np.int64)
    status[V < 2] = FEW_VIEWS
    for nv in np.unique(V[V >= 2]):
        ls = np.nonzero(V == nv)[0]
        vidx = np.stack([views[l] for l in ls])            # (n, V)
        kf = view_kf[vidx]; px = view_px[vidx]
        P, C = _cams(R, t, kf, fx, fy, cx, cy)
        X = xyz[ls].astype(np.float64)
        d = _norm3(X[:, None, :] - C)
        best = np.zeros(len(ls))
        with np.errstate(all="ignore"):
            for i in range(nv):
                for j in range(i + 1, nv):
                    ang = np.arctan2(_norm3(C[:, i] - C[:, j]), (d[:, i] + d[:, j]) / 2.0)
                    best = np.where(ang > best, ang, best)
        info["max_angle"][ls] = best
        ok = ~(best < MIN_PARALLAX)
        status[ls[~ok]] = LOW_PARALLAX
        ls, P, px = ls[ok], P[ok], px[ok]
        if len(ls) == 0:
            continue
        u = px[..., 0].astype(np.float64); v = px[..., 1].astype(np.float64)
        At = np.zeros((len(ls), 4, 2 * nv))
        for k in range(4):
            At[:, k, 0::2] = u * P[..., 2, k] - P[..., 0, k]
            At[:, k, 1::2] = v * P[..., 2, k] - P[..., 1, k]
        x, sweeps = jacobi_null_vectors(At)
        info["x"][ls] = x; info["sweeps"][ls] = sweeps
        with np.errstate(all="ignore"):
            if nv == 2:
                w = x[:, 3].astype(np.float32)
                deg = w == 0
                newp = x[:, :3].astype(np.float32) / w[:, None]
            else:
                deg = x[:, 3] == 0
                newp = (x[:, :3] / x[:, 3:4]).astype(np.float32)
            Y = newp.astype(np.float64)
            total = np.zeros(len(ls)); count = np.zeros(len(ls), np.int64)
            for s in range(nv):
                pr = [P[:, s, r, 0] * Y[:, 0] + P[:, s, r, 1] * Y[:, 1] + P[:, s, r, 2] * Y[:, 2] + P[:, s, r, 3] * 1.0 for r in range(3)]
                front = pr[2] > 0
                ru = (pr[0] / pr[2]).astype(np.float32); rv = (pr[1] / pr[2]).astype(np.float32)
                dx = (px[:, s, 0] - ru).astype(np.float32); dy = (px[:, s, 1] - rv).astype(np.float32)
                dx = dx.astype(np.float64); dy = dy.astype(np.float64)
                err = np.sqrt(dx * dx + dy * dy)
                total = np.where(front, total + err, total); count += front
            reproj = (count > 0) & (total / np.maximum(count, 1).astype(np.float64) > 2.0)
        z = newp[:, 2].astype(np.float64)
        depth_ok = (z > 0.1) & (z < 10.0)
        st = np.where(deg, DEGENERATE, np.where(reproj, REPROJECTION, np.where(depth_ok, UPDATED, DEPTH)))
        status[ls] = st
        upd = st == UPDATED
        out[ls[upd]] = newp[upd]
    return (out, status, info) if details else (out, status)


# ---- scenes ------------------------------------------------------------------------------------------------------------------
def rot(ax, ay, az):
    cx_, sx = np.cos(ax), np.sin(ax); cy_, sy = np.cos(ay), np.sin(ay); cz, sz = np.cos(az), np.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx_, -sx], [0, sx, cx_]]); Ry = np.array([[cy_, 0, sy], [0, 1, 0], [-sy, 0, cy_]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


K4 = (525.0, 525.0, 319.5, 239.5)


def keyframes(rng, nkf, span=2.0):
    """world -> camera poses of nkf cameras spread over a span x span/2 patch, looking roughly along +z"""
    R = np.zeros((nkf, 9)); t = np.zeros((nkf, 3)); Cs = np.zeros((nkf, 3))
    for k in range(nkf):
        Rk = rot(*rng.uniform(-0.05, 0.05, 3))
        C = np.array([rng.uniform(-span / 2, span / 2), rng.uniform(-span / 4, span / 4), rng.uniform(-0.2, 0.2)])
        R[k] = Rk.ravel(); t[k] = -Rk @ C; Cs[k] = C
    return R, t, Cs


def project(R, t, kf, X, K=K4):
    fx, fy, cx, cy = K
    Rk = R[kf].reshape(3, 3); xc = Rk @ X + t[kf]
    return np.array([fx * xc[0] / xc[2] + cx, fy * xc[1] / xc[2] + cy])


def random_landmarks(rng, R, t, nlm, vmin, vmax, noise=0.5, perturb=0.05, skip=0.0, depth=(2.0, 6.0)):
    """nlm landmarks with vmin..vmax views each on random distinct keyframes; pixels with Gaussian noise (px), input positions off by
    `perturb` metres, a fraction `skip` of extra views with view_kf = -1.  -> (offsets, view_kf, view_px, xyz_in, X_true)"""
    nkf = len(R)
    offs = [0]; vkf = []; vpx = []; xyz = []; Xt = []
    for _ in range(nlm):
        X = np.array([rng.uniform(-1.5, 1.5), rng.uniform(-1.0, 1.0), rng.uniform(*depth)])
        nv = int(rng.integers(vmin, vmax + 1))
        kfs = rng.choice(nkf, size=nv, replace=nv > nkf)
        for k in kfs:
            if skip and rng.random() < skip:
                vkf.append(-1); vpx.append(rng.uniform(0, 640, 2))
            vkf.append(int(k)); vpx.append(project(R, t, k, X) + rng.normal(0, noise, 2) if noise else project(R, t, k, X))
        offs.append(len(vkf))
        xyz.append(X + rng.normal(0, perturb, 3)); Xt.append(X)
    return (np.array(offs, np.int64), np.array(vkf, np.int32), np.array(vpx, np.float32).reshape(-1, 2), np.array(xyz, np.float32).reshape(-1, 3),
            np.array(Xt).reshape(-1, 3))


def status_scenes():
    """one landmark per status (and the zero-count quirk: landmark 6), on one set of keyframes -> (R, t, offsets, view_kf, view_px, xyz, expected)"""
    # keyframes 0-5 look along +z; 6-8 are turned round (they look along -z), so a point in front of 0-5 is behind them
    centres = [(-0.5, 0, 0), (0.5, 0, 0), (0, 0.4, 0), (0, 0, 0), (0, 0, 0), (0.8, -0.3, 0.1), (-0.5, 0, 0), (0.5, 0, 0), (0, 0.4, 0)]
    rots = [rot(0, 0, 0), rot(0.02, -0.03, 0), rot(-0.01, 0.02, 0.01), rot(0, 0, 0), rot(0, 0.3, 0), rot(0.01, 0.01, -0.02),
            rot(0, np.pi, 0), rot(0.02, np.pi, 0), rot(0, np.pi - 0.03, 0.01)]
    R = np.zeros((len(rots), 9)); t = np.zeros((len(rots), 3))
    for k in range(len(rots)):
        R[k] = rots[k].ravel(); t[k] = -rots[k] @ np.array(centres[k])
    Xa = np.array([0.2, -0.1, 3.0])
    views = []; xyz = []; exp = []

    def add(kfs, pxs, X0, e):
        views.append(list(zip(kfs, pxs))); xyz.append(X0); exp.append(e)
    add([0], [project(R, t, 0, Xa)], Xa + 0.01, FEW_VIEWS)                                   # one view
    add([-1, -1, 1], [project(R, t, 0, Xa)] * 3, Xa + 0.01, FEW_VIEWS)                      # one view after skips
    add([-1, -1], [project(R, t, 0, Xa)] * 2, Xa + 0.01, FEW_VIEWS)                         # zero views after skips
    add([3, 4], [project(R, t, 3, Xa), project(R, t, 4, Xa)], Xa + 0.01, LOW_PARALLAX)      # pure rotation (same centre)
    add([0, 1, 2], [project(R, t, 0, Xa), project(R, t, 1, Xa), project(R, t, 2, Xa) + np.array([40.0, -25.0])], Xa + 0.01,
        REPROJECTION)                                                                          # one outlier pixel
    Xf = np.array([0.5, 0.3, 14.0])
    add([0, 1, 5], [project(R, t, k, Xf) for k in (0, 1, 5)], np.array([0.5, 0.3, 3.0]), DEPTH)   # z > 10 (gate passes at 3 m)
    Xb = np.array([0.1, 0.0, 3.0])                                    # behind every camera: no view counts, accepted (the quirk)
    add([6, 7, 8], [project(R, t, k, Xb) for k in (6, 7, 8)], Xb + 0.05, UPDATED)
    add([0, 1, 2, 5], [project(R, t, k, Xa) + np.array([0.3, -0.2]) for k in (0, 1, 2, 5)], Xa + 0.02, UPDATED)
    add([0, 1], [project(R, t, 0, Xa), project(R, t, 1, Xa)], Xa + 0.02, UPDATED)
    offs = np.cumsum([0] + [len(v) for v in views]).astype(np.int64)
    vkf = np.array([k for v in views for k, _ in v], np.int32)
    vpx = np.array([p for v in views for _, p in v], np.float32).reshape(-1, 2)
    return R, t, offs, vkf, vpx, np.array(xyz, np.float32), exp
