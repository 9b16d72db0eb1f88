"""Landmark culling restated (include/dvslam_hip.h "Landmark culling") over backend_ref.BackendRef with dicts and Python sets: the tracking
statistics as {landmark id: [visible, found]}, their alignment to the map, the recording of one map-tracking call, the two rules and the
apply with dvs_backend_prune's cascade.  PARITY UNPINNED: the reference has no counterpart.  Everything is integers and total orders, so the
device is compared bit for bit.  The scenes of tests/test_gpu_landmark_culling.py are built here too; the conditions they must meet are
asserted without a GPU in tests/test_landmark_culling_cpu.py."""
import functools
import numpy as np
import backend_ref as br
import map_track_ref as mr

INT32_MAX = 2 ** 31 - 1
DEFAULTS = dict(found_ratio_pct=25, min_visible=4, weak_age_kf=2, weak_max_views=1)
REASON_F, REASON_W = 1, 2


def check_params(P):
    if set(P) != set(DEFAULTS):
        raise TypeError(sorted(set(P) ^ set(DEFAULTS)))
    if P["found_ratio_pct"] > 100 or P["min_visible"] < 1 or P["weak_max_views"] < 0:
        raise ValueError(P)


# ---------------------------------------------------------------------------------------------------- the map
def landmarks(ref):
    """{id: landmark} over every class"""
    return {lid: lm for d in ref.db.values() for lid, lm in d.items()}


def ref_from_tables(keyframes, lms, obs, counts, filtered=(br.PERSON,)):
    """a BackendRef that holds what the getters of a handle returned: the restatement then runs on the device's own map"""
    ref = br.BackendRef(br.FX, br.FY, br.CX, br.CY, filtered=filtered)
    for k, f in enumerate(keyframes["frame_id"]):
        a, b = keyframes["obs_offsets"][k], keyframes["obs_offsets"][k + 1]
        ref.kfs.append(dict(frame=int(f), R=keyframes["R"][k].reshape(9).copy(), t=keyframes["t"][k].copy(), stamp=int(keyframes["stamp_ns"][k]),
                            obs_ids=[int(i) for i in keyframes["obs_ids"][a:b]]))
    for i in range(len(obs["id"])):
        ref.obs.append(dict(id=int(obs["id"][i]), frame=int(obs["frame_id"][i]), px=obs["px"][i].copy(), desc=obs["desc"][i].copy(), cls=int(obs["class_id"][i]),
                            lm=int(obs["landmark_id"][i])))
    for s in range(len(lms["id"])):
        a, b = lms["obs_offsets"][s], lms["obs_offsets"][s + 1]
        ref.db.setdefault(int(lms["class_id"][s]), {})[int(lms["id"][s])] = dict(
            id=int(lms["id"][s]), cls=int(lms["class_id"][s]), pos=lms["xyz"][s].copy(), desc=lms["desc"][s].copy(), obs_ids=[int(i) for i in lms["obs_ids"][a:b]],
            count=int(lms["observation_count"][s]), last_seen=int(lms["last_seen_ns"][s]))
    ref.next_obs, ref.next_lm = counts["next_observation_id"], counts["next_landmark_id"]
    return ref


def views(ref):
    """{id: (n, age_kf)}: n = the observation rows naming the landmark; age_kf = (nkf - 1) - the keyframe index of the first of them, in table
    order, whose frame is a keyframe of the map; -1 without one"""
    kf_of = {}
    for k, kf in enumerate(ref.kfs):
        kf_of.setdefault(kf["frame"], k)
    ids = set(landmarks(ref))
    n = {lid: 0 for lid in ids}; first = {}
    for o in ref.obs:
        if o["lm"] in ids:
            n[o["lm"]] += 1
            if o["lm"] not in first and o["frame"] in kf_of:
                first[o["lm"]] = kf_of[o["frame"]]
    return {lid: (n[lid], (len(ref.kfs) - 1) - first[lid] if lid in first else -1) for lid in ids}


# ---------------------------------------------------------------------------------------------------- the statistics
def align(ref, stats):
    """the statistics of exactly the map's ids: a known id keeps its counters, a new one starts at 0 / 0, the others are dropped"""
    return {lid: list(stats.get(lid, (0, 0))) for lid in landmarks(ref)}


def record(stats, ids, visible_flags, kp_lm_id, kp_inlier, status):
    """one map-tracking call: ids / visible_flags per row handed to the tracker; kp_lm_id / kp_inlier per keypoint (the id of the landmark
    it kept or -1, and whether the pair ended as an inlier).  Told from the keypoints' side: a landmark is found iff some keypoint kept it
    as an inlier."""
    if status != mr.OK:
        return
    found = {int(l) for l, i in zip(kp_lm_id, kp_inlier) if int(l) >= 0 and i}
    for lid, vis in zip(ids, visible_flags):
        lid = int(lid)
        if not vis or lid not in stats or stats[lid][0] == INT32_MAX:
            continue
        stats[lid][0] += 1
        if lid in found:
            stats[lid][1] += 1


def stats_table(ref, stats):
    """dvs_backend_get_landmark_stats"""
    st, v = align(ref, stats), views(ref)
    ids = sorted(st)
    return dict(id=np.array(ids, np.uint64), visible=np.array([st[i][0] for i in ids], np.int32), found=np.array([st[i][1] for i in ids], np.int32),
                n_views=np.array([v[i][0] for i in ids], np.int32), age_kf=np.array([v[i][1] for i in ids], np.int32))


# ---------------------------------------------------------------------------------------------------- the cull
def rule(visible, found, n, age_kf, P):
    """the first rule that holds: 1 F, 2 W, 0 none"""
    if P["found_ratio_pct"] > 0 and visible >= P["min_visible"] and found * 100 < P["found_ratio_pct"] * visible:
        return REASON_F
    if P["weak_age_kf"] >= 0 and age_kf >= P["weak_age_kf"] and n <= P["weak_max_views"]:
        return REASON_W
    return 0


def decide(ref, stats, **params):
    """-> (culled ids ascending, their reasons, dict(n_landmarks, n_by_ratio, n_weak))"""
    P = dict(DEFAULTS, **params)
    check_params(P)
    st, v = align(ref, stats), views(ref)
    ids, why = [], []
    for lid in sorted(st):
        r = rule(st[lid][0], st[lid][1], v[lid][0], v[lid][1], P)
        if r:
            ids.append(lid); why.append(r)
    return ids, why, dict(n_landmarks=len(st), n_by_ratio=why.count(REASON_F), n_weak=why.count(REASON_W))


def apply(ref, stats, culled_ids):
    """the prune cascade on ref and stats, in place -> dict(n_landmarks_removed, n_observations_removed, n_keyframes_touched)"""
    gone_lm = set(int(i) for i in culled_ids)
    if not gone_lm:
        return dict(n_landmarks_removed=0, n_observations_removed=0, n_keyframes_touched=0)
    for d in ref.db.values():
        for lid in [l for l in d if l in gone_lm]:
            del d[lid]
    ref._rows = {}
    gone_ob = {o["id"] for o in ref.obs if o["lm"] in gone_lm}
    ref.obs = [o for o in ref.obs if o["id"] not in gone_ob]
    touched = 0
    for kf in ref.kfs:
        keep = [i for i in kf["obs_ids"] if i not in gone_ob]
        touched += len(keep) != len(kf["obs_ids"])
        kf["obs_ids"] = keep
    for lid in gone_lm:
        stats.pop(lid, None)
    return dict(n_landmarks_removed=len(gone_lm), n_observations_removed=len(gone_ob), n_keyframes_touched=touched)


def cull(ref, stats, do_apply=True, **params):
    """dvs_backend_cull_landmarks -> the dict MappingBackend.cull_landmarks returns"""
    ids, why, out = decide(ref, stats, **params)
    out.update(apply(ref, stats, ids) if do_apply else dict(n_landmarks_removed=0, n_observations_removed=0, n_keyframes_touched=0))
    out.update(culled_id=np.array(ids, np.uint64), culled_reason=np.array(why, np.int32))
    return out


# ---------------------------------------------------------------------------------------------------- the recording scene
GRID = 32.0                    # pixels between two projections: more than 2 * radius = 30
SHIFT = 16.0                   # the moved prior puts every projection half a grid step to the right
DEPTH = 2.0
IDENTITY_Q = (0.0, 0.0, 0.0, 1.0)
KIND_A, KIND_B, KIND_C = 0, 1, 2
DECOY_DY = [8.0] * 7 + [12.5, 13.5, 14.5, -5.0, -7.0, -9.0, -11.0, -13.0, -14.5]
N_DECOYS = len(DECOY_DY)       # 16: at least min_matches = 15


@functools.lru_cache(maxsize=None)
def record_scene(n_lm, seed=31):
    """one keyframe at the origin that creates n_lm landmarks, and one frame seen from the origin.  Landmark j is of group j % 4 -> A, B, C, C:
    A and B sit at depth 2 on a 32-pixel grid of projections (more than 2 * radius apart); every A has a keypoint at its projection with the
    landmark's own descriptor, no B has a keypoint within radius; the C are behind the camera (even) or far outside the image (odd).
    The first N_DECOYS of the A also have a DECOY keypoint with their descriptor, half a grid step to the right and DECOY_DY pixels down:
    outside every window under the true prior (|dx| > 15 from every grid column), inside its landmark's window under the prior moved by
    SHIFT pixels, where no true keypoint is.  Seven decoys agree on one more shift of 8 pixels, the other nine lie at least 4.5 pixels from
    that and from each other's pairs: the robust rounds settle on the seven, and seven inliers are fewer than min_inliers = 10.  That is
    the FEW_INLIERS case.
    -> dict(kf, kind, kps, kdesc, n_true, R, t, t_moved)"""
    rng = np.random.default_rng(seed + n_lm)
    P = track_params()
    gx, gy = np.meshgrid(np.arange(24.0, 616.0, GRID), np.arange(24.0, 456.0, GRID))
    spots = np.stack([gx.ravel(), gy.ravel()], 1)
    spots = spots[rng.permutation(len(spots))]
    kind = np.array([(KIND_A, KIND_B, KIND_C, KIND_C)[j % 4] for j in range(n_lm)])
    assert (kind != KIND_C).sum() <= len(spots)
    desc = mr.random_descriptors(rng, n_lm)
    xyz = np.zeros((n_lm, 3)); px = np.zeros((n_lm, 2)); s = 0
    for j in range(n_lm):
        if kind[j] == KIND_C:
            xyz[j] = (rng.uniform(-1, 1), rng.uniform(-1, 1), -DEPTH) if j % 8 < 4 else (40.0 + j, 1.0, DEPTH)
            px[j] = (10.0, 10.0)
        else:
            px[j] = spots[s]; s += 1
            xyz[j] = ((px[j, 0] - P.cx) * DEPTH / P.fx, (px[j, 1] - P.cy) * DEPTH / P.fy, DEPTH)
    a = np.flatnonzero(kind == KIND_A)
    decoy = px[a[:N_DECOYS]] + np.stack([SHIFT + np.array([0.0] * 7 + list(rng.uniform(-0.9, 0.9, N_DECOYS - 7))), np.array(DECOY_DY)], 1)
    order = rng.permutation(len(a) + N_DECOYS)
    kxy = np.concatenate([px[a], decoy])[order]
    kdesc = np.concatenate([desc[a], desc[a[:N_DECOYS]]])[order]
    kps = mr.keypoints(kxy)
    n_true = np.flatnonzero(order < len(a))               # the keypoints at exact projections
    kf = dict(frame_id=500, stamp=(10, 0), t=np.zeros(3), q=IDENTITY_Q, xyz=xyz, px=px, desc=desc, det=[])
    return dict(kf=kf, kind=kind, kps=kps, kdesc=kdesc, true_kp=n_true, R=np.eye(3), t=np.zeros(3), t_moved=np.array([-SHIFT * DEPTH / P.fx, 0.0, 0.0]))


def track_params(**kw):
    """the map tracker's parameters for the backend scenes' camera"""
    return mr.Params(480, 640, br.FX, br.FY, br.CX, br.CY, **kw)


# ---------------------------------------------------------------------------------------------------- the moved object
OBJECT_N, STATIC_N, OBJECT_NKF = 40, 90, 3
OBJECT_FRAME0 = 800


@functools.lru_cache(maxsize=None)
def object_scene(seed=41):
    """three keyframes stepping sideways see STATIC_N static points and OBJECT_N points of an object, every point in every keyframe (three
    views each, so rule W cannot fire); then the object is gone: the later frames, taken at the last keyframe's pose, hold the static points'
    keypoints only.  -> (keyframes, query): query = dict(R, t, kps, kdesc, is_object per scene point, X, D)"""
    rng = np.random.default_rng(seed)
    n = STATIC_N + OBJECT_N
    X = np.stack([rng.uniform(-0.9, 0.9, n), rng.uniform(-0.7, 0.7, n), rng.uniform(2.5, 4.5, n)], 1)
    X[STATIC_N:] = np.stack([rng.uniform(-0.3, 0.3, OBJECT_N), rng.uniform(-0.3, 0.3, OBJECT_N), rng.uniform(2.6, 3.0, OBJECT_N)], 1)     # the block
    D = mr.random_descriptors(rng, n)
    out = []
    for k in range(OBJECT_NKF):
        t = np.array([0.15 * k, 0.0, 0.0])
        u = br.FX * (-X[:, 0] + t[0]) / X[:, 2] + br.CX; v = br.FY * (-X[:, 1] + t[1]) / X[:, 2] + br.CY
        px = np.stack([u, v], 1) + rng.normal(0, 0.05, (n, 2))
        out.append(dict(frame_id=OBJECT_FRAME0 + k, stamp=(10 + k, 0), t=t, q=br.Q_Z180, xyz=X + rng.normal(0, 0.002, (n, 3)), px=px, desc=D.copy(), det=[]))
    t = out[-1]["t"]
    u = br.FX * (-X[:STATIC_N, 0] + t[0]) / X[:STATIC_N, 2] + br.CX; v = br.FY * (-X[:STATIC_N, 1] + t[1]) / X[:STATIC_N, 2] + br.CY
    perm = rng.permutation(STATIC_N)
    kps = mr.keypoints(np.stack([u, v], 1)[perm])
    is_object = np.arange(n) >= STATIC_N
    return out, dict(R=np.diag([-1.0, -1.0, 1.0]), t=t.copy(), kps=kps, kdesc=D[:STATIC_N][perm].copy(), is_object=is_object, X=X, D=D)


def object_ids(ref, q):
    """the ids of the landmarks the object's points created: by descriptor, which no two points share"""
    by_desc = {q["D"][j].tobytes(): bool(q["is_object"][j]) for j in range(len(q["D"]))}
    return {lid for lid, lm in landmarks(ref).items() if by_desc[lm["desc"].tobytes()]}
