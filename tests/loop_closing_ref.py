"""The rule of include/dvslam_hip.h "Loop closing on the map" (dvs_backend_get_anchors, dvs_backend_build_pose_graph, dvs_backend_fuse,
dvs_backend_close_loop) restated sequentially over a backend_ref.BackendRef: plain loops over dicts and lists, one landmark and one
observation after the other, nothing of the kernels' structure (no flags, no tiles, no atomics).  The pose-graph solve and the point
correction are pose_graph_ref's.  Also the scene of the tests: a camera that goes out, comes back to its start with a drifted pose and
sees the first keyframe's points again."""
import copy
import functools
import numpy as np

import backend_ref as br
import pose_graph_ref as pr

f32 = np.float32
FUSE_DEFAULTS = dict(max_descriptor_distance=50.0, max_reprojection_distance=5.0, fuse_neighbours=2)


def _kf_index(ref):
    out = {}
    for k, kf in enumerate(ref.kfs):
        out.setdefault(kf["frame"], k)
    return out


def _landmarks(ref):
    """id -> landmark dict over all classes"""
    return {lid: lm for d in ref.db.values() for lid, lm in d.items()}


def anchors(ref):
    """(ids ascending uint64, int32 keyframe index of each landmark's lowest-id observation still in the observation table, -1 without)"""
    kf_of = _kf_index(ref)
    first = {}
    for o in sorted(ref.obs, key=lambda o: o["id"]):
        first.setdefault(o["lm"], kf_of.get(o["frame"], -1))
    ids = sorted(_landmarks(ref))
    return np.array(ids, np.uint64), np.array([first.get(i, -1) for i in ids], np.int32)


def relative_pose(Ra, ta, Rb, tb):
    """(rvec, tvec) of Z = T_a^-1 T_b: R_z = R_a^T R_b, t_z = R_a^T (t_b - t_a), every product a left-to-right sum of Python floats"""
    Ra = [[float(Ra[r][c]) for c in range(3)] for r in range(3)]; Rb = [[float(Rb[r][c]) for c in range(3)] for r in range(3)]
    Q = np.array([[Ra[0][r] * Rb[0][c] + Ra[1][r] * Rb[1][c] + Ra[2][r] * Rb[2][c] for c in range(3)] for r in range(3)], np.float64)
    d = [float(tb[k]) - float(ta[k]) for k in range(3)]
    tz = np.array([Ra[0][r] * d[0] + Ra[1][r] * d[1] + Ra[2][r] * d[2] for r in range(3)], np.float64)
    return pr.so3_log(Q)[0], tz


def build_pose_graph(ref, loops, w):
    """loops: [(query frame id, entry frame id, rvec, tvec, w_rot, w_trans)]; w = (odo_w_rot, odo_w_trans) -> the arrays of a pr.Graph"""
    kf_of = _kf_index(ref)
    n = len(ref.kfs)
    if n < 2:
        raise ValueError("fewer than two keyframes")
    R = np.array([kf["R"] for kf in ref.kfs], np.float64).reshape(-1, 3, 3); t = np.array([kf["t"] for kf in ref.kfs], np.float64).reshape(-1, 3)
    fixed = np.zeros(n, np.uint8); fixed[0] = 1
    ei, ej, rv, tv, wr, wt = [], [], [], [], [], []
    for k in range(n - 1):
        a, b = relative_pose(R[k], t[k], R[k + 1], t[k + 1])
        ei.append(k); ej.append(k + 1); rv.append(a); tv.append(b); wr.append(float(w[0])); wt.append(float(w[1]))
    for q, e, rvec, tvec, w_rot, w_trans in loops:
        if q not in kf_of or e not in kf_of or kf_of[q] == kf_of[e] or not (w_rot > 0 and w_trans > 0):
            raise ValueError("bad loop")
        ei.append(kf_of[q]); ej.append(kf_of[e]); rv.append(np.array(rvec, np.float64)); tv.append(np.array(tvec, np.float64)); wr.append(float(w_rot)); wt.append(float(w_trans))
    return dict(R=R, t=t, fixed=fixed, ei=np.array(ei, np.int32), ej=np.array(ej, np.int32), rvec=np.array(rv, np.float64).reshape(-1, 3),
                tvec=np.array(tv, np.float64).reshape(-1, 3), w_rot=np.array(wr, np.float64), w_trans=np.array(wt, np.float64))


def in_front(X, R, t):
    """c2 > 0 for c = R^T (X - t), in reprojection_error's arithmetic"""
    d0, d1, d2 = float(X[0]) - t[0], float(X[1]) - t[1], float(X[2]) - t[2]
    return R[2] * d0 + R[5] * d1 + R[8] * d2 > 0


def fuse(ref, q_frame, entry_frames, params=None, apply=True):
    """-> dict(n_sources, n_targets, n_proposals, n_fused, pairs=[(survivor id, removed id, e)] in ascending removed id)"""
    P = dict(FUSE_DEFAULTS, **(params or {}))
    kf_of = _kf_index(ref)
    entry_frames = [int(f) for f in entry_frames]
    if q_frame not in kf_of or any(f not in kf_of for f in entry_frames) or q_frame in entry_frames or len(set(entry_frames)) != len(entry_frames) \
            or not 1 <= len(entry_frames) <= 64:
        raise ValueError("bad frames")
    lms = _landmarks(ref)
    kq = ref.kfs[kf_of[q_frame]]
    R, t = kq["R"], kq["t"]
    q_obs = [o for o in ref.obs if o["frame"] == q_frame and o["lm"] in lms]
    targets = set(o["lm"] for o in q_obs)
    named = set(o["lm"] for o in ref.obs if o["frame"] in entry_frames and o["lm"] in lms)
    sources = sorted(named - targets)
    proposals = {}                                     # target id -> [(e, source id)]
    for a in sources:
        A = lms[a]
        if not in_front(A["pos"], R, t):
            continue
        best = None
        for o in q_obs:
            if A["cls"] != o["cls"]:
                continue
            e = br.reprojection_error(o["px"], A["pos"], R, t, *ref.K)
            if not e < P["max_reprojection_distance"]:
                continue
            if not br.hamming(A["desc"], o["desc"]) < P["max_descriptor_distance"]:
                continue
            if best is None or (e, o["id"]) < best[:2]:
                best = (e, o["id"], o["lm"])
        if best is not None:
            proposals.setdefault(best[2], []).append((best[0], a))
    pairs = []
    for b, props in proposals.items():
        e, a = min(props)
        pairs.append((min(a, b), max(a, b), e))
    pairs.sort(key=lambda p: p[1])
    out = dict(n_sources=len(sources), n_targets=len(targets), n_proposals=sum(len(v) for v in proposals.values()), n_fused=len(pairs), pairs=pairs)
    if apply:
        for keep, gone, _ in pairs:
            K, G = lms[keep], lms[gone]
            K["count"] += G["count"]; K["last_seen"] = max(K["last_seen"], G["last_seen"])
            for o in ref.obs:
                if o["lm"] == gone:
                    o["lm"] = keep
            K["obs_ids"] = sorted(set(K["obs_ids"]) | set(G["obs_ids"]))
            del ref.db[G["cls"]][gone]
        ref._rows = {}
    return out


def close_loop(ref, loops, w, pgo_params=None, fuse_params=None):
    """dvs_backend_close_loop on the restatement: pose_graph_ref.solve, poses written back, pose_graph_ref.correct_points with the anchors,
    then one fusion per loop.  -> dict(summary fields, n_landmarks_moved, fuse counts, pairs of every loop)"""
    g = build_pose_graph(ref, loops, w)
    G = pr.Graph(g["R"], g["t"], g["fixed"], g["ei"], g["ej"], g["rvec"], g["tvec"], g["w_rot"], g["w_trans"])
    s = pr.solve(G, pgo_params)
    out = dict(termination=s["termination"], n_nodes=G.N, n_edges=G.E, n_landmarks_moved=0, n_sources=0, n_targets=0, n_proposals=0, n_fused=0, pairs=[])
    if s["termination"] == 2:
        return out
    ids, anc = anchors(ref)
    lms = _landmarks(ref)
    xyz = np.array([lms[int(i)]["pos"] for i in ids], f32).reshape(-1, 3)
    # the "before" rotations are the ones given; the current ones are made from the quaternion, as dvs_pgo_get_nodes returns them
    moved = pr.correct_points(xyz, anc, g["R"], g["t"], s["R"], s["t"])
    for k, i in enumerate(ids):
        lms[int(i)]["pos"] = moved[k].copy()
    for k, kf in enumerate(ref.kfs):
        kf["R"] = s["R"][k].reshape(9).copy(); kf["t"] = s["t"][k].copy()
    out["n_landmarks_moved"] = int((anc >= 0).sum())
    if fuse_params is not None:
        P = dict(FUSE_DEFAULTS, **fuse_params)
        n = len(ref.kfs)
        for e in range(G.N - 1, G.E):
            q, entry = int(g["ei"][e]), int(g["ej"][e])
            E = [ref.kfs[k]["frame"] for k in range(max(0, entry - P["fuse_neighbours"]), min(n - 1, entry + P["fuse_neighbours"]) + 1) if k != q]
            if not E:
                continue
            r = fuse(ref, ref.kfs[q]["frame"], E, P, True)
            for k in ("n_sources", "n_targets", "n_proposals", "n_fused"):
                out[k] += r[k]
            out["pairs"].append(r["pairs"])
    return out


def adopt_geometry(ref, keyframes, landmarks):
    """the keyframe poses and landmark positions of a handle's tables (MappingBackend.keyframes() / .landmarks()) put into the restatement:
    the device's pose-graph solve agrees with pose_graph_ref.solve to a tolerance, not to the bit, so a bit-for-bit fusion test starts
    both sides from the handle's geometry"""
    assert [kf["frame"] for kf in ref.kfs] == [int(f) for f in keyframes["frame_id"]]
    for k, kf in enumerate(ref.kfs):
        kf["R"] = np.array(keyframes["R"][k], np.float64).reshape(9).copy(); kf["t"] = np.array(keyframes["t"][k], np.float64).copy()
    lms = _landmarks(ref)
    assert sorted(lms) == [int(i) for i in landmarks["id"]]
    for k, i in enumerate(landmarks["id"]):
        lms[int(i)]["pos"] = np.array(landmarks["xyz"][k], f32).copy()


# ---- the scene ---------------------------------------------------------------------------------------------------------------------
FX = FY = 600.0; CX, CY = 320.0, 240.0
NKF = 12
STEP, LANE = 0.6, 2.6                 # metres between keyframes; the way back runs LANE metres beside the way out (no common points)
DRIFT = np.array([0.19, 0.06, 0.0])   # the reported translation of the last keyframe is off by this much (0.2 m); it grows linearly


def true_positions():
    """out along x (keyframes 0 .. 5), back along the other lane (6 .. 10), and the last keyframe beside the first"""
    pos = [(STEP * k, 0.0) for k in range(6)] + [(STEP * (11 - k), LANE) for k in range(6, 11)] + [(0.05, 0.02)]
    return np.array([(x, y, 0.0) for x, y in pos])


def make_scene(seed=3, per_m2=40.0, pixel_noise=0.3, position_noise=0.01, max_flips=10):
    """-> (keyframes, truth): keyframes as backend_ref.make_scene's dicts (no detections: one class), with the drifted pose and the
    landmark positions the front end would report with it; truth = dict(t = true translations, point = per keyframe the world point index
    of every observation, loop = (query frame, entry frame, rvec, tvec) the true relative pose of the last keyframe against the first)"""
    rng = np.random.default_rng(seed)
    x0, x1, y0, y1 = -1.7, 5 * STEP + 1.7, -1.3, LANE + 1.3
    npts = int(per_m2 * (x1 - x0) * (y1 - y0))
    X = np.stack([rng.uniform(x0, x1, npts), rng.uniform(y0, y1, npts), rng.uniform(2.6, 3.4, npts)], 1)
    D = rng.integers(0, 256, (npts, 32), dtype=np.uint8)
    T = true_positions()
    out, point = [], []
    for k in range(NKF):
        t = T[k]
        xc = np.stack([-(X[:, 0] - t[0]), -(X[:, 1] - t[1]), X[:, 2]], 1)          # R = diag(-1, -1, 1) (backend_ref.Q_Z180)
        u = FX * xc[:, 0] / xc[:, 2] + CX; v = FY * xc[:, 1] / xc[:, 2] + CY
        vis = np.nonzero((u > 8) & (u < 632) & (v > 8) & (v < 472))[0]
        vis = vis[rng.permutation(len(vis))]
        px = np.stack([u[vis], v[vis]], 1) + rng.normal(0, pixel_noise, (len(vis), 2))
        desc = D[vis].copy()
        for r in range(len(vis)):
            for b in rng.choice(256, rng.integers(0, max_flips + 1), replace=False):
                desc[r, b >> 3] ^= np.uint8(1 << (b & 7))
        drift = DRIFT * (k / (NKF - 1))
        xyz = X[vis] + drift + rng.normal(0, position_noise, (len(vis), 3))
        out.append(dict(frame_id=200 + k, stamp=(10 + 2 * k, 0), t=t + drift, q=br.Q_Z180, xyz=xyz, px=px, desc=desc, det=[]))
        point.append(vis)
    R = br.quat_to_R(br.Q_Z180).reshape(3, 3)
    rvec, tvec = relative_pose(R, T[NKF - 1], R, T[0])
    return out, dict(t=T, point=point, loop=(200 + NKF - 1, 200, rvec, tvec))


def new_ref():
    return br.BackendRef(FX, FY, CX, CY)


def add(x, kf):
    return x.add_keyframe(kf["frame_id"], kf["stamp"], kf["t"], kf["q"], kf["xyz"], kf["px"], kf["desc"], kf["det"])


@functools.lru_cache(maxsize=None)
def scene():
    """make_scene() with its defaults, made once per process; read-only"""
    return make_scene()


@functools.lru_cache(maxsize=None)
def _scene_run():
    ref = new_ref()
    results, anc = [], []
    for kf in scene()[0]:
        results.append(add(ref, kf)); anc.append(anchors(ref))
    return ref, results, anc


def scene_ref():
    """-> (a fresh copy of the restatement after every keyframe of scene(), the result records): the run itself is made once per process"""
    ref, results, _ = _scene_run()
    return copy.deepcopy(ref), results


def scene_anchors():
    """anchors() after every keyframe of scene()"""
    return _scene_run()[2]


def scene_loop(w_rot=300.0, w_trans=200.0):
    q, e, rvec, tvec = scene()[1]["loop"]
    return [(q, e, rvec, tvec, w_rot, w_trans)]


ODO_W = (100.0, 100.0)
