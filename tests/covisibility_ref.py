"""The rule of include/dvslam_hip.h "Covisibility" (dvs_backend_covisibility, dvs_backend_get_local_window, dvs_backend_local_ba,
dvs_backend_track_frame_local) restated over the arrays the getters return (MappingBackend.keyframes() / landmarks() / observations(), a
backend_ref.BackendRef's tables, or hand-made dicts of the same columns): Python sets and sorted tuples, one keyframe and one row after the
other, nothing of the kernels' structure (no CSR, no histogram, no flags).  PARITY UNPINNED: the rule is the library's own.
Also the scenes of the tests: the hub scene, whose incidence is designed, and backend_ref.make_scene() followed by a fusion."""
import functools
import numpy as np

import backend_ref as br
import loop_closing_ref as lc

f32 = np.float32
DEFAULTS = dict(min_weight=15, max_neighbours=10, max_fixed=32, ba_max_iterations=20)


def check_params(P):
    if P["min_weight"] < 1 or not 0 <= P["max_neighbours"] <= 62 or not 0 <= P["max_fixed"] <= 63 or P["max_neighbours"] + 1 + P["max_fixed"] > 64 \
            or P["ba_max_iterations"] < 1:
        raise ValueError("bad parameters")


def tables(ref):
    """a BackendRef's tables in the order the functions below take them"""
    return ref.keyframe_table(), ref.landmark_table(), ref.observation_table()


def observes(keyframes, landmarks, observations):
    """-> [S_k]: per keyframe (table order) the set of landmark ids it observes"""
    slot = {int(f): k for k, f in enumerate(keyframes["frame_id"])}
    held = set(int(i) for i in landmarks["id"])
    S = [set() for _ in slot]
    for f, l in zip(observations["frame_id"], observations["landmark_id"]):
        if int(f) in slot and int(l) in held:
            S[slot[int(f)]].add(int(l))
    return S


def weights(S):
    return np.array([[len(a & b) for b in S] for a in S], np.int32).reshape(len(S), len(S))


def neighbours(W, a, theta):
    """-> [(index, weight)] ordered by weight descending, then index ascending"""
    return [(b, -w) for w, b in sorted((-int(W[a][b]), b) for b in range(len(W)) if b != a and W[a][b] >= theta)]


def graph(keyframes, landmarks, observations, theta):
    """what MappingBackend.covisibility(theta) returns"""
    if theta < 1:
        raise ValueError("bad parameters")
    W = weights(observes(keyframes, landmarks, observations))
    offs, idx, wt = [0], [], []
    for a in range(len(W)):
        for b, w in neighbours(W, a, theta):
            idx.append(b); wt.append(w)
        offs.append(len(idx))
    return dict(weights=W, nb_offsets=np.array(offs, np.int64), nb_index=np.array(idx, np.int32), nb_weight=np.array(wt, np.int32))


def local_set(S, W, r, P):
    """-> (free keyframes ascending, U ascending)"""
    free = sorted([r] + [b for b, _ in neighbours(W, r, P["min_weight"])[:P["max_neighbours"]]])
    U = set()
    for k in free:
        U |= S[k]
    return free, sorted(U)


def local_window(keyframes, landmarks, observations, ref_frame_id, SW=None, **params):
    """what MappingBackend.local_window(ref_frame_id, **params) returns, plus kf_index (the window's keyframes as table indices).
    SW: (observes(...), weights(...)) of the same tables, if the caller has them already"""
    P = dict(DEFAULTS, **params)
    check_params(P)
    slot = {int(f): k for k, f in enumerate(keyframes["frame_id"])}
    if int(ref_frame_id) not in slot:
        raise ValueError("unknown frame")
    r = slot[int(ref_frame_id)]
    S = SW[0] if SW else observes(keyframes, landmarks, observations)
    W = SW[1] if SW else weights(S)
    free, U = local_set(S, W, r, P)
    Uset = set(U)
    ranked = sorted((-len(S[c] & Uset), c) for c in range(len(S)) if c not in free and len(S[c] & Uset) >= 1)
    fixed = [c for _, c in ranked[:P["max_fixed"]]]
    if not fixed:
        fixed = [free[0]]                                                # the gauge
    window = sorted(set(free) | set(fixed))
    row_of = {l: j for j, l in enumerate(U)}
    seen, rows, left = set(), [], 0
    for i, (f, l) in enumerate(zip(observations["frame_id"], observations["landmark_id"])):
        k = slot.get(int(f), -1)
        if k not in window or int(l) not in row_of:
            continue
        if (k, int(l)) in seen:
            left += 1
            continue
        seen.add((k, int(l)))
        rows.append(i)
    lm_row = {int(i): j for j, i in enumerate(landmarks["id"])}
    lrows = [lm_row[l] for l in U]
    return dict(kf_index=np.array(window, np.int32), kf_frame_id=np.asarray(keyframes["frame_id"], np.uint64)[window],
                kf_R=np.asarray(keyframes["R"], np.float64).reshape(-1, 3, 3)[window], kf_t=np.asarray(keyframes["t"], np.float64).reshape(-1, 3)[window],
                kf_fixed=np.array([1 if k in fixed else 0 for k in window], np.uint8), kf_weight=np.array([W[r][k] for k in window], np.int32),
                obs_px=np.asarray(observations["px"], f32).reshape(-1, 2)[rows], obs_landmark_id=np.asarray(observations["landmark_id"], np.uint64)[rows],
                obs_class=np.asarray(observations["class_id"], np.int32)[rows], obs_frame_id=np.asarray(observations["frame_id"], np.uint64)[rows],
                obs_lm_index=np.array([row_of[int(observations["landmark_id"][i])] for i in rows], np.int32),
                lm_id=np.asarray(landmarks["id"], np.uint64)[lrows], lm_class=np.asarray(landmarks["class_id"], np.int32)[lrows],
                lm_xyz=np.asarray(landmarks["xyz"], f32).reshape(-1, 3)[lrows], n_left_out=left)


def local_map(keyframes, landmarks, observations, ref_frame_id, SW=None, **params):
    """-> (xyz, desc, id) of U: what dvs_backend_track_frame_local hands to the map tracker"""
    w = local_window(keyframes, landmarks, observations, ref_frame_id, SW, **dict(params, max_fixed=0))
    lm_row = {int(i): j for j, i in enumerate(landmarks["id"])}
    rows = [lm_row[int(l)] for l in w["lm_id"]]
    return w["lm_xyz"], np.asarray(landmarks["desc"], np.uint8).reshape(-1, 32)[rows], w["lm_id"].astype(np.int64)


def local_ba_problem(window, fx, fy, cx, cy):
    """the problem dvs_backend_local_ba assembles from a local window -> (problem dict as BAProblem takes it, mask over U of the landmarks in
    the problem, n_dropped)"""
    from global_ba_ref import pose_from_rt
    slot = {int(f): k for k, f in enumerate(window["kf_frame_id"])}
    count = np.bincount(window["obs_lm_index"], minlength=len(window["lm_id"]))
    used = count >= 2
    new_row = np.cumsum(used) - 1
    rows = [i for i, l in enumerate(window["obs_lm_index"]) if used[l]]
    K, L = len(slot), int(used.sum())
    q = np.zeros((K, 4)); t = np.zeros((K, 3))
    for k in range(K):
        q[k], t[k] = pose_from_rt(window["kf_R"][k], window["kf_t"][k])
    prob = dict(K=K, L=L, q=q, t=t, X=window["lm_xyz"][used].astype(np.float64).reshape(L, 3),
                cam_idx=np.array([slot[int(window["obs_frame_id"][i])] for i in rows], np.int32),
                lm_idx=np.array([new_row[window["obs_lm_index"][i]] for i in rows], np.int32),
                uv=window["obs_px"][rows].astype(np.float64).reshape(-1, 2), pose_fixed=window["kf_fixed"].copy(), lm_fixed=np.zeros(L, np.uint8),
                fx=fx, fy=fy, cx=cx, cy=cy, sigma=1.0, huber=1.345)
    return prob, used, len(window["obs_lm_index"]) - len(rows)


# ---- scenes ------------------------------------------------------------------------------------------------------------------------
HUB_NKF = 300
HUB = 7                                  # the hub keyframe's index; frame ids are HUB_FRAME0 + index
HUB_FRAME0 = 1000
HUB_BLOCK = 20                           # landmarks a cluster shares: weight 21 with the landmark everybody sees, above theta = 15
_OTHERS = [k for k in range(HUB_NKF) if k != HUB]
# clusters of keyframe indices that share one block each: 65 + the hub, 65, 64, 2 -> neighbour lists of 65, 64, 63 and 1 at theta = 15
HUB_CLUSTERS = [_OTHERS[0:65], _OTHERS[65:130], _OTHERS[130:194], _OTHERS[194:196]]
HUB_LEAVES = _OTHERS[196:]               # 103 keyframes that see the common landmark and three of the hub's own: no neighbour at theta = 15
HUB_LEAF = HUB_LEAVES[40]
HUB_OWN = 3 * len(HUB_LEAVES)            # the hub's own landmarks: |S_hub| = 1 + 309 + 20 = 330 > 256
HUB_LENGTHS_15 = {HUB: 65, HUB_CLUSTERS[0][0]: 65, HUB_CLUSTERS[0][-1]: 65, HUB_CLUSTERS[1][0]: 64, HUB_CLUSTERS[1][-1]: 64, HUB_CLUSTERS[2][0]: 63,
                  HUB_CLUSTERS[2][-1]: 63, HUB_CLUSTERS[3][0]: 1, HUB_CLUSTERS[3][1]: 1, HUB_LEAVES[0]: 0, HUB_LEAVES[-1]: 0}


def hub_incidence():
    """-> per keyframe the list of world point indices it sees.  Point 0: everybody; 1 .. HUB_OWN: the hub's own, three per leaf;
    then one block per cluster."""
    blocks = [list(range(1 + HUB_OWN + HUB_BLOCK * c, 1 + HUB_OWN + HUB_BLOCK * (c + 1))) for c in range(len(HUB_CLUSTERS))]
    sees = [[0] for _ in range(HUB_NKF)]
    sees[HUB] += list(range(1, 1 + HUB_OWN)) + blocks[0]
    for c, members in enumerate(HUB_CLUSTERS):
        for k in members:
            sees[k] += blocks[c]
    for j, k in enumerate(HUB_LEAVES):
        sees[k] += [1 + 3 * j, 2 + 3 * j, 3 + 3 * j]
    return sees


@functools.lru_cache(maxsize=None)
def hub_scene(seed=21):
    """-> keyframes as backend_ref.make_scene's dicts (no detections: one class).  Every world point has its own random descriptor (pairs
    are about 128 bits apart, far beyond the gate of 50) and is seen at its exact projection with its exact position, so the association
    follows hub_incidence().  The camera steps 4 mm sideways per keyframe; every point is inside every image."""
    rng = np.random.default_rng(seed)
    sees = hub_incidence()
    npts = 1 + max(max(s) for s in sees)
    X = np.stack([rng.uniform(-0.6, 1.8, npts), rng.uniform(-0.8, 0.8, npts), rng.uniform(3.2, 5.0, npts)], 1)
    D = rng.integers(0, 256, (npts, 32), dtype=np.uint8)
    out = []
    for k in range(HUB_NKF):
        t = np.array([0.004 * k, 0.001 * k, 0.0])
        idx = np.array(sees[k])
        idx = idx[rng.permutation(len(idx))]
        xc = np.stack([-X[idx, 0] + t[0], -X[idx, 1] + t[1], X[idx, 2]], 1)                     # Q_Z180, as backend_ref.make_scene
        px = np.stack([br.FX * xc[:, 0] / xc[:, 2] + br.CX, br.FY * xc[:, 1] / xc[:, 2] + br.CY], 1)
        assert (px[:, 0] > 8).all() and (px[:, 0] < 632).all() and (px[:, 1] > 8).all() and (px[:, 1] < 472).all()
        out.append(dict(frame_id=HUB_FRAME0 + k, stamp=(10 + k, 0), t=t, q=br.Q_Z180, xyz=X[idx].copy(), px=px, desc=D[idx].copy(), det=[]))
    return out


def hub_conditions(g1, g15):
    """the conditions the GPU tests rely on, on graph(..., 1) and graph(..., 15) of the hub scene"""
    W = g1["weights"]
    n1 = np.diff(g1["nb_offsets"]); n15 = np.diff(g15["nb_offsets"])
    assert W.shape == (HUB_NKF, HUB_NKF) and (W == W.T).all()
    assert W[HUB][HUB] == 1 + HUB_OWN + HUB_BLOCK > 256                   # more landmarks than one trip of the workgroup
    assert (n1 == HUB_NKF - 1).all() and HUB_NKF - 1 > 256                # a landmark seen by everybody: a view segment above 64, lists above 256
    assert {k: int(n15[k]) for k in HUB_LENGTHS_15} == HUB_LENGTHS_15
    assert sorted(set(n15.tolist())) == [0, 1, 63, 64, 65]
    off = W[~np.eye(HUB_NKF, dtype=bool)]
    assert len(set(off.tolist())) <= 4 and (off == 1).sum() > 1000 and (off == 21).sum() > 1000      # many equal weights


# backend_ref.make_scene() sees every world point once per keyframe, so a fusion at the default gates merges only duplicates of one point and
# no keyframe ends up naming a landmark twice.  With the descriptor gate open and 20 pixels of reprojection the last keyframe's landmarks
# also absorb landmarks of NEIGHBOURING points, which the earlier keyframes saw beside them: those keyframes then name the survivor twice.
FUSED_QUERY, FUSED_ENTRIES = 109, (100, 101, 102, 103, 104)
FUSED_PARAMS = dict(max_reprojection_distance=20.0, max_descriptor_distance=257.0)


def fused_ref():
    """make_scene() as it is through the restatement (PERSON filtered, as the backend tests run it), then the fusion above"""
    ref = scene_ref(br.make_scene(), filtered=(br.PERSON,))
    out = lc.fuse(ref, FUSED_QUERY, FUSED_ENTRIES, FUSED_PARAMS)
    return ref, out


class IncidenceRef(br.BackendRef):
    """BackendRef without re-triangulation, for the hub scene only: its observations are exact, so a landmark's position stays within
    rounding of where it was created whether it is re-triangulated or not, and the association — all the covisibility rule reads — is the
    same.  (Re-triangulating a landmark of 300 views after each of them takes the plain reference two minutes.)"""

    def triangulate(self, lm):
        return False


def scene_ref(keyframes, filtered=(), cls=br.BackendRef):
    ref = cls(br.FX, br.FY, br.CX, br.CY, filtered=filtered)
    for kf in keyframes:
        lc.add(ref, kf)
    return ref


def repeated_pairs(keyframes, landmarks, observations):
    """how many observation rows are a later row of their (keyframe, landmark) pair"""
    seen, n = set(), 0
    held = set(int(i) for i in landmarks["id"])
    for f, l in zip(observations["frame_id"], observations["landmark_id"]):
        if int(l) in held:
            n += (int(f), int(l)) in seen
            seen.add((int(f), int(l)))
    return n
