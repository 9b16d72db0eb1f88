"""The rule of include/dvslam_hip.h "Landmark refresh" (dvs_backend_refresh_landmarks, dvs_backend_get_landmark_geometry, the gated
dvs_maptrack_* calls) restated over the arrays the getters return: numpy and Python sets, one landmark and one view after the other,
nothing of the kernels' structure (no CSR, no bins, no bisection).  PARITY UNPINNED: the rule is the library's own.
Also the scenes of the tests: maps whose landmarks have designed numbers of views, the drift scene, the wall scene and the gate scene."""
import functools
import math
import numpy as np

import backend_ref as br
import covisibility_ref as cr
import map_track_ref as mr

DEFAULT_GATES = dict(cos_min=0.5, range_factor=2.0)
NO_VIEW_ID, NO_VIEW_MEDIAN = np.uint64(2**64 - 1), -1
NEAR, FAR, BACK, ANGLE = 0, 1, 2, 3
NORMAL_BOUND = lambda m: (m + 32) * 2.0 ** -53          # absolute, per normal component
RANGE_BOUND = 16 * 2.0 ** -53                            # relative, dmin and dmax


# ---------------------------------------------------------------------------------------------------- views and the selection
def views(landmarks, observations):
    """-> per landmark row the observation rows naming it, in table order"""
    row = {int(i): s for s, i in enumerate(landmarks["id"])}
    out = [[] for _ in row]
    for i, l in enumerate(observations["landmark_id"]):
        if int(l) in row:
            out[row[int(l)]].append(i)
    return out


def distances(desc):
    """n x 32 uint8 -> n x n Hamming distances"""
    d = np.asarray(desc, np.uint8).reshape(-1, 32)
    return np.unpackbits(d[:, None, :] ^ d[None, :, :], axis=2).sum(2).astype(np.int64)


def select(desc):
    """the chosen view of descriptors desc (n >= 1) -> (index, its median)"""
    D = distances(desc)
    n = len(D)
    best = None
    for i in range(n):
        med = sorted(int(v) for v in D[i])[(n - 1) // 2]
        if best is None or (med, i) < best:
            best = (med, i)
    return best[1], best[0]


def scope_rows(keyframes, landmarks, observations, scope_frame_id):
    """the landmark rows in scope: all, or S_k of that keyframe ("Covisibility")"""
    if scope_frame_id is None:
        return set(range(len(landmarks["id"])))
    frames = [int(f) for f in keyframes["frame_id"]]
    if int(scope_frame_id) not in frames:
        raise ValueError("unknown frame")
    S = cr.observes(keyframes, landmarks, observations)[frames.index(int(scope_frame_id))]
    return set(s for s, i in enumerate(landmarks["id"]) if int(i) in S)


def refresh(keyframes, landmarks, observations, scope_frame_id=None, min_views=1, update_descriptors=1):
    """what MappingBackend.refresh_landmarks returns, and the landmark descriptor column after it"""
    if min_views < 1:
        raise ValueError("bad parameters")
    V = views(landmarks, observations)
    scope = scope_rows(keyframes, landmarks, observations, scope_frame_id)
    desc = np.array(landmarks["desc"], np.uint8).reshape(-1, 32).copy()
    odesc = np.asarray(observations["desc"], np.uint8).reshape(-1, 32)
    res = dict(n_in_scope=len(scope), n_changed=0, n_without_views=0, max_views=0)
    for s in sorted(scope):
        n = len(V[s])
        res["max_views"] = max(res["max_views"], n)
        if n == 0:
            res["n_without_views"] += 1
        if n == 0 or n < min_views:
            continue
        i, _ = select(odesc[V[s]])
        if odesc[V[s][i]].tobytes() != desc[s].tobytes():
            res["n_changed"] += 1
            if update_descriptors:
                desc[s] = odesc[V[s][i]]
    return res, desc


# ---------------------------------------------------------------------------------------------------- geometry
def geometry(keyframes, landmarks, observations, real=float):
    """what MappingBackend.landmark_geometry returns; real = float: the rule's FP64, every expression as the header writes it;
    real = numpy.longdouble: the same in extended precision (normal and range then come back as longdouble arrays)"""
    V = views(landmarks, observations)
    slot = {int(f): k for k, f in enumerate(keyframes["frame_id"])}
    kt = np.asarray(keyframes["t"], np.float64).reshape(-1, 3)
    xyz = np.asarray(landmarks["xyz"], np.float32).reshape(-1, 3)
    odesc = np.asarray(observations["desc"], np.uint8).reshape(-1, 32)
    n = len(V)
    dt = np.float64 if real is float else np.longdouble
    normal = np.zeros((n, 3), dt); rng = np.zeros((n, 2), dt); cnt = np.zeros(n, np.int32)
    oid = np.full(n, NO_VIEW_ID, np.uint64); med = np.full(n, NO_VIEW_MEDIAN, np.int32)
    sqrt = math.sqrt if real is float else np.sqrt
    for s in range(n):
        X = [real(float(v)) for v in xyz[s]]
        acc = [real(0.0)] * 3
        dmin = dmax = real(0.0)
        m = 0
        for i in V[s]:
            k = slot.get(int(observations["frame_id"][i]), -1)
            if k < 0:
                continue
            d = [X[c] - real(float(kt[k][c])) for c in range(3)]
            r = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
            if not (r > 0 and np.isfinite(r)):
                continue
            acc = [acc[c] + d[c] / r for c in range(3)]
            dmin = r if m == 0 or r < dmin else dmin
            dmax = r if m == 0 or r > dmax else dmax
            m += 1
        if m:
            acc = [a / real(m) for a in acc]
        normal[s] = acc; rng[s] = (dmin, dmax); cnt[s] = m
        if V[s]:
            i, md = select(odesc[V[s]])
            oid[s], med[s] = observations["id"][V[s][i]], md
    return dict(normal=normal, range=rng, n_counted=cnt, best_obs_id=oid, best_median=med)


# ---------------------------------------------------------------------------------------------------- gates
def gate(X, O, N, dmin, dmax, m, cos_min, range_factor, real=float):
    """-> the first failing test (NEAR, FAR, BACK, ANGLE) or -1; the terms of every comparison as (lhs, rhs) pairs for the margins"""
    if m <= 0:
        return -1, []
    X = [real(float(np.float32(v))) for v in X]; O = [real(float(v)) for v in O]; N = [real(float(v)) for v in N]
    p = [X[c] - O[c] for c in range(3)]
    q = (p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]
    s = (p[0] * N[0] + p[1] * N[1]) + p[2] * N[2]
    a = real(float(dmin)) / real(range_factor); b = real(float(dmax)) * real(range_factor)
    cc = real(cos_min) * real(cos_min)
    terms = [(q, a * a), (q, b * b), (s, real(0.0)), (s * s, cc * q)]
    g = NEAR if q < a * a else FAR if q > b * b else BACK if s < 0 else ANGLE if s * s < cc * q else -1
    return g, terms


# landmarks at X = (0, 0, 2) seen from O = 0 (q = 4), every number a small dyadic rational: ((N, dmin, dmax, m, cos_min, range_factor), gate)
EXACT_GATE_CASES = [
    (([0.0, 0.0, 0.5], 4.0, 1.0, 1, 0.5, 2.0), -1),       # a * a = 4, b * b = 4, s * s = 1 = cc * q: equality on three tests, none holds
    (([0.0, 0.0, 0.5], 4.5, 8.0, 1, 0.5, 2.0), NEAR),     # a * a = 5.0625 > 4
    (([0.0, 0.0, 0.5], 1.0, 0.875, 1, 0.5, 2.0), FAR),    # b * b = 3.0625 < 4
    (([0.0, 0.0, -0.5], 4.0, 1.0, 1, 0.5, 2.0), BACK),    # s = -1
    (([0.0, 0.0, 0.0], 4.0, 1.0, 1, 0.5, 2.0), ANGLE),    # s = 0 is not < 0; s * s = 0 < 1
    (([0.0, 0.0, 0.0], 4.0, 1.0, 1, 0.0, 2.0), -1),       # cos_min = 0: 0 < 0 is false
    (([0.0, 0.0, 0.4375], 4.0, 1.0, 1, 0.5, 2.0), ANGLE), # s = 0.875, s * s = 0.765625 < 1
    (([0.0, 0.0, 0.5], 2.0, 2.0, 1, 0.5, 1.0), -1),       # range_factor = 1: a * a = b * b = 4
    (([0.0, 0.0, 0.5], 2.25, 8.0, 1, 0.5, 1.0), NEAR),
    (([0.0, 0.0, -0.5], 9.0, 0.5, 0, 1.0, 2.0), -1),      # m == 0 passes whatever the geometry says
    (([0.0, 0.0, 1.0], 4.0, 1.0, 2, 1.0, 2.0), -1),       # cos_min = 1, s * s = 4 = q
]


def gates(xyz, O, normal, rng, ncnt, cos_min=0.5, range_factor=2.0, real=float):
    """-> (per landmark the gate that fires or -1, the four counts)"""
    g = np.array([gate(xyz[j], O, normal[j], rng[j][0], rng[j][1], int(ncnt[j]), cos_min, range_factor, real)[0] for j in range(len(xyz))], np.int32).reshape(-1)
    return g, np.array([(g == k).sum() for k in range(4)], np.int32)


def gate_margin(xyz, O, normal, rng, ncnt, cos_min=0.5, range_factor=2.0):
    """the smallest relative distance of any landmark to any gate it is tested at, in longdouble"""
    ld = np.longdouble
    worst = math.inf
    for j in range(len(xyz)):
        g, terms = gate(xyz[j], O, normal[j], rng[j][0], rng[j][1], int(ncnt[j]), cos_min, range_factor, ld)
        for k, (lhs, rhs) in enumerate(terms):
            scale = max(abs(lhs), abs(rhs)) if k != 2 else math.sqrt(float(terms[0][0])) * max(float(np.abs(np.asarray(normal[j], np.float64)).max()), 1e-300)
            worst = min(worst, float(abs(lhs - rhs) / scale))
            if g == k:
                break                                   # the later tests are not reached
    return worst


def search_gated(P, R, t, xyz, ldesc, kps, kdesc, normal, rng, ncnt, cos_min=0.5, range_factor=2.0, search=mr.search_grid):
    """stages 1-3 with the gate in stage 1: map_track_ref's search over the landmarks that pass (the search treats every landmark on its
    own), the records of the others as those of a landmark that is not visible -> (rec, kp_lm, kp_dist, gate counts)"""
    g, counts = gates(xyz, [float(v) for v in np.asarray(t, np.float64).reshape(3)], normal, rng, ncnt, cos_min, range_factor)
    keep = np.flatnonzero(g < 0)
    Rcw, tcw = mr.pose_cw(R, t)
    rec = np.zeros(len(xyz), mr.LM_RECORD)
    rec["best_k"] = rec["d_best"] = rec["d_second"] = -1
    if len(keep):
        rec[keep] = search(P, Rcw, tcw, np.asarray(xyz)[keep], np.asarray(ldesc)[keep], kps, kdesc)
    kp_lm, kp_dist = mr.assign(rec, len(kps))
    return rec, kp_lm, kp_dist, counts


# ---------------------------------------------------------------------------------------------------- scenes
def flip(desc, bits):
    d = np.array(desc, np.uint8).copy()
    for b in bits:
        d[int(b) >> 3] ^= np.uint8(1 << (int(b) & 7))
    return d


def _keyframe(frame_id, k, t, X, D, order, det=()):
    """a keyframe of the hub scene's kind (Q_Z180, t in the x-y plane): exact positions at their exact projections"""
    idx = np.asarray(order, np.int64)
    xc = np.stack([-X[idx, 0] + t[0], -X[idx, 1] + t[1], X[idx, 2]], 1)
    px = np.stack([br.FX * xc[:, 0] / xc[:, 2] + br.CX, br.FY * xc[:, 1] / xc[:, 2] + br.CY], 1)
    assert (px[:, 0] > 8).all() and (px[:, 0] < 632).all() and (px[:, 1] > 8).all() and (px[:, 1] < 472).all()
    return dict(frame_id=frame_id, stamp=(10 + k, 0), t=np.asarray(t, np.float64), q=br.Q_Z180, xyz=X[idx].copy(), px=px, desc=np.asarray(D, np.uint8), det=list(det))


# the numbers of views around every change of path: the segment of eight lanes, the wavefront, the LDS tile of 256, and the hub scene's 300
VIEW_COUNTS = [1, 2, 3, 4, 7, 8, 9, 63, 64, 65, 255, 256, 257, 300]
VIEWS_FRAME0 = 5000
VIEWS_LONELY = VIEWS_FRAME0 + 300         # the keyframe that is culled to leave a landmark with no view


@functools.lru_cache(maxsize=None)
def views_scene(seed=5):
    """-> (keyframes, counts): 301 keyframes; point j is seen by the first counts[j] of the first 300.  The counts are VIEW_COUNTS and then 46
    more in 1..20, so that the lists of the first two paths are longer than one wavefront and one workgroup take.  Every view's descriptor
    is within 20 bits of the point's base descriptor, so within 40 < 49 of the landmark's (the first view's); odd points draw their views
    from three variants only: identical descriptors, rows with many equal medians.  The last keyframe sees point 0 and a point of its
    own: culled with drop_orphans = 0, it leaves that landmark in the table with no view."""
    rng = np.random.default_rng(seed)
    counts = VIEW_COUNTS + [1 + (7 * j) % 20 for j in range(46)]
    npts = len(counts) + 1
    X = np.stack([rng.uniform(-0.6, 1.8, npts), rng.uniform(-0.8, 0.8, npts), rng.uniform(3.2, 5.0, npts)], 1)
    base = rng.integers(0, 256, (npts, 32), dtype=np.uint8)
    pool = [[flip(base[j], rng.choice(256, 20, replace=False)) for _ in range(3)] for j in range(npts)]
    out = []
    for k in range(300):
        idx = [j for j, c in enumerate(counts) if k < c]
        idx = [idx[i] for i in rng.permutation(len(idx))]
        D = [pool[j][int(rng.integers(0, 3))] if j % 2 else flip(base[j], rng.choice(256, int(rng.integers(0, 21)), replace=False)) for j in idx]
        out.append(_keyframe(VIEWS_FRAME0 + k, k, (0.004 * k, 0.001 * k, 0.0), X, D, idx))
    lonely = npts - 1
    out.append(_keyframe(VIEWS_LONELY, 300, (1.2, 0.3, 0.0), X, [base[13], base[lonely]], [13, lonely]))
    return out, counts


def leave_a_landmark_without_views(mb):
    """culls VIEWS_LONELY from a handle that holds views_scene(): every other keyframe protected, nothing dropped"""
    frames = mb.keyframes()["frame_id"]
    rep = mb.cull_keyframes(None, [int(f) for f in frames if int(f) != VIEWS_LONELY], True, min_observers=1, redundancy_percent=0, keep_recent=0, drop_orphans=0)
    assert rep["n_culled"] == 1 and rep["n_landmarks_removed"] == 0
    return rep


# ---- the drift scene: eight keyframes, each view of a drifting point 6 more bits from the first than the one before; the query frame 54
DRIFT_NKF, DRIFT_STEP, DRIFT_QUERY_BITS = 8, 6, 54
DRIFT_N, DRIFT_STATIC = 40, 30            # drifting points, and points whose descriptor never changes (they keep tracking alive)
DRIFT_FRAME0 = 7000


@functools.lru_cache(maxsize=None)
def drift_scene(seed=11):
    """-> (keyframes, query): query = dict(R, t, kps, kdesc, drifting: the keypoints that show drifting points).  Points on a grid of image
    positions 48 pixels apart, so no search window (radius 15) holds two.  View v of a drifting point has the first 6 v bits of the point's own
    bit order flipped; the query has the first 54.  D[i][j] = 6 |i - j|: the medians are 18, 12, 12, 12, 12, 12, 12, 18, so view 1 is chosen,
    48 bits from the query, while the first view — the landmark's descriptor until a refresh — is 54 away: outside max_hamming = 50."""
    rng = np.random.default_rng(seed)
    n = DRIFT_N + DRIFT_STATIC
    gx, gy = np.meshgrid(np.arange(60.0, 600.0, 48.0), np.arange(60.0, 440.0, 48.0))
    uv = np.stack([gx.ravel(), gy.ravel()], 1)[rng.permutation(gx.size)[:n]]
    z = rng.uniform(3.5, 4.5, n)
    X = np.stack([-(uv[:, 0] - br.CX) * z / br.FX, -(uv[:, 1] - br.CY) * z / br.FY, z], 1)
    base = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    order = [rng.permutation(256) for _ in range(n)]
    out = []
    for k in range(DRIFT_NKF):
        idx = [int(i) for i in rng.permutation(n)]
        D = [flip(base[j], order[j][:DRIFT_STEP * k]) if j < DRIFT_N else base[j] for j in idx]
        out.append(_keyframe(DRIFT_FRAME0 + k, k, (0.004 * k, 0.001 * k, 0.0), X, D, idx))
    tq = np.array([0.004 * DRIFT_NKF, 0.001 * DRIFT_NKF, 0.0])
    R = np.asarray(br.quat_to_R(br.Q_Z180), np.float64).reshape(3, 3)
    xc = (X - tq) @ R                                   # R^T (X - t), R symmetric
    xy = np.stack([br.FX * xc[:, 0] / xc[:, 2] + br.CX, br.FY * xc[:, 1] / xc[:, 2] + br.CY], 1) + rng.normal(0, 0.3, (n, 2))
    kps = mr.keypoints(xy)
    kdesc = np.array([flip(base[j], order[j][:DRIFT_QUERY_BITS]) if j < DRIFT_N else base[j] for j in range(n)], np.uint8)
    return out, dict(R=R, t=tq, kps=kps, kdesc=kdesc, drifting=np.arange(n) < DRIFT_N)


def track_params(**kw):
    """the map tracker's parameters for the backend scenes' camera"""
    return mr.Params(480, 640, br.FX, br.FY, br.CX, br.CY, **kw)


def matched_keypoints(P, R, t, landmarks, kps, kdesc, desc=None):
    """the keypoints that keep a landmark, by map_track_ref's stages 1-3 on a landmark table -> bool per keypoint"""
    Rcw, tcw = mr.pose_cw(R, t)
    rec = mr.search_grid(P, Rcw, tcw, landmarks["xyz"], landmarks["desc"] if desc is None else desc, kps, kdesc)
    return mr.assign(rec, len(kps))[0] >= 0


# ---- the wall scene: a wall at z = 4 seen from z = 0 (three keyframes looking along +z) and from z = 8 (three looking along -z)
WALL_N = 48
WALL_FRAME0 = 8000
Q_Y180 = (0.0, 1.0, 0.0, 0.0)             # R = diag(-1, 1, -1): with t_y = 0, R X + t (triangulate) and R^T (X - t) (reprojectPoint) agree


@functools.lru_cache(maxsize=None)
def wall_scene(seed=13):
    """-> (keyframes, query).  Front point j and back point j are 0.1 m apart on the wall (12.5 pixels from 4 m: beyond the association's
    5 pixels, inside the search radius of 15) and 30 bits apart, so from the front a back point's landmark finds the front point's keypoint
    at distance 30 < 50 with nothing else in its window: it proposes, unless its viewing direction keeps it out."""
    rng = np.random.default_rng(seed)
    gx, gy = np.meshgrid(np.arange(80.0, 580.0, 60.0), np.arange(70.0, 420.0, 60.0))
    uv = np.stack([gx.ravel(), gy.ravel()], 1)[:WALL_N]
    F = np.stack([-(uv[:, 0] - br.CX) * 4.0 / br.FX, -(uv[:, 1] - br.CY) * 4.0 / br.FY, np.full(WALL_N, 4.0)], 1)
    B = F + np.array([0.1, 0.0, 0.0])
    DF = rng.integers(0, 256, (WALL_N, 32), dtype=np.uint8)
    DB = np.array([flip(DF[j], rng.choice(256, 30, replace=False)) for j in range(WALL_N)], np.uint8)
    out = []
    for k in range(3):
        out.append(_keyframe(WALL_FRAME0 + k, k, (0.01 * k, 0.0, 0.0), F, DF, np.arange(WALL_N)))
    Rb = np.asarray(br.quat_to_R(Q_Y180), np.float64).reshape(3, 3)
    for k in range(3):
        t = np.array([0.01 * k, 0.0, 8.0])
        xc = (B - t) @ Rb
        px = np.stack([br.FX * xc[:, 0] / xc[:, 2] + br.CX, br.FY * xc[:, 1] / xc[:, 2] + br.CY], 1)
        assert (xc[:, 2] > 3.9).all() and (px[:, 0] > 8).all() and (px[:, 0] < 632).all() and (px[:, 1] > 8).all() and (px[:, 1] < 472).all()
        out.append(dict(frame_id=WALL_FRAME0 + 3 + k, stamp=(20 + k, 0), t=t, q=Q_Y180, xyz=B.copy(), px=px, desc=DB.copy(), det=[]))
    tq = np.array([0.03, 0.0, 0.0])
    R = np.asarray(br.quat_to_R(br.Q_Z180), np.float64).reshape(3, 3)
    xc = (F - tq) @ R
    xy = np.stack([br.FX * xc[:, 0] / xc[:, 2] + br.CX, br.FY * xc[:, 1] / xc[:, 2] + br.CY], 1) + rng.normal(0, 0.4, (WALL_N, 2))
    return out, dict(R=R, t=tq, kps=mr.keypoints(xy), kdesc=DF.copy())


# ---- the gate scene: map_track_ref.search_scene with host-made geometry; landmark j's kind is j % 6
GATE_KINDS = ("pass", "near", "far", "back", "angle", "uncounted")


def gate_scene(P, n_lm, n_kp, seed):
    """-> (xyz, ldesc, kps, kdesc, normal, range, ncnt, R, t): the geometry is made so that landmark j passes (j % 6 == 0), fails exactly the
    near / far / back-facing / angle test first (1 .. 4), or has m == 0 with a geometry that would fail (5).  Every margin is random and
    wide: tests/test_landmark_refresh_cpu.py asserts 1e-9 relative in longdouble."""
    rng = np.random.default_rng(seed)
    R, t = mr.FRAME_R, mr.FRAME_T
    xyz, ldesc, kps, kdesc = mr.search_scene(P, n_lm, n_kp, seed, R, t)
    normal = np.zeros((n_lm, 3)); rg = np.zeros((n_lm, 2)); cnt = np.zeros(n_lm, np.int32)
    for j in range(n_lm):
        p = xyz[j].astype(np.float64) - t
        r = float(np.linalg.norm(p))
        e = p / r
        side = np.cross(e, [0.0, 1.0, 0.0]); side /= np.linalg.norm(side)
        kind = j % 6
        c = rng.uniform(0.75, 0.95)                     # the cosine between the viewing direction and the normal; |normal| in 0.8 .. 1
        if kind == 4:
            c = rng.uniform(0.05, 0.4)
        n = (c * e + math.sqrt(1 - c * c) * side) * rng.uniform(0.8, 1.0)
        lo, hi = r * rng.uniform(0.6, 0.9), r * rng.uniform(1.1, 1.6)
        if kind == 1:
            lo, hi = r * rng.uniform(2.5, 4.0), r * 5.0
        if kind == 2:
            lo, hi = r * 0.1, r * rng.uniform(0.2, 0.4)
        if kind == 3:
            n = -n
        if kind == 5:
            n, lo, hi = -n, r * 3.0, r * 5.0
        normal[j], rg[j], cnt[j] = n, (lo, hi), 0 if kind == 5 else 1 + j % 7
    return xyz, ldesc, kps, kdesc, normal, rg, cnt, R, t
