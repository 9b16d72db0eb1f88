"""The rule of include/dvslam_hip.h "Keyframe culling" (dvs_backend_cull_keyframes) restated over the arrays the getters return
(MappingBackend.keyframes() / landmarks() / observations(), a backend_ref.BackendRef's tables, or hand-made dicts of the same columns):
Python sets, one candidate after the other with no prefilter, nothing of the kernels' structure (no CSR, no flags, no compaction).
PARITY UNPINNED: the rule is the library's own.  `one_shot` tests every candidate against the initial counts instead: it is NOT the rule,
and is here only to show that the scenes of the tests tell the two apart."""
import numpy as np

import covisibility_ref as cr

DEFAULTS = dict(min_observers=3, redundancy_percent=90, min_weight=15, keep_recent=2, max_cull=0, drop_orphans=1)
OUT, PROTECTED, KEPT, CULLED = 0, 1, 2, 3


def check_params(P):
    if P["min_observers"] < 1 or not 0 <= P["redundancy_percent"] <= 99 or P["min_weight"] < 1 or P["keep_recent"] < 0 or P["max_cull"] < 0:
        raise ValueError("bad parameters")


def redundant(S_k, c, P):
    """-> (n_k, R_k, is k redundant) under the counts c"""
    n = len(S_k)
    R = sum(1 for l in S_k if c[l] - 1 >= P["min_observers"])
    return n, R, n >= 1 and 100 * R > P["redundancy_percent"] * n


def decide(keyframes, landmarks, observations, ref_frame_id=None, protected=(), one_shot=False, **params):
    """-> the report of MappingBackend.cull_keyframes(ref_frame_id, protected, apply=False, **params), without the two "removed" counts"""
    P = dict(DEFAULTS, **params)
    check_params(P)
    frames = [int(f) for f in keyframes["frame_id"]]
    slot = {f: k for k, f in enumerate(frames)}
    if any(int(f) not in slot for f in protected) or (ref_frame_id is not None and int(ref_frame_id) not in slot):
        raise ValueError("unknown frame")
    nkf = len(frames)
    S = cr.observes(keyframes, landmarks, observations)
    c = {}
    for s in S:
        for l in s:
            c[l] = c.get(l, 0) + 1
    first = [redundant(S[k], c, P) for k in range(nkf)]
    prot = set([0] if nkf else []) | set(range(max(0, nkf - P["keep_recent"]), nkf)) | set(slot[int(f)] for f in protected)
    if ref_frame_id is None:
        scope = set(range(nkf))
    else:
        r = slot[int(ref_frame_id)]
        prot.add(r)
        scope = set(b for b, _ in cr.neighbours(cr.weights(S), r, P["min_weight"]))
    state = [PROTECTED if k in prot else KEPT if k in scope else OUT for k in range(nkf)]
    candidates = [k for k in range(nkf) if state[k] == KEPT]
    culled = []
    for k in candidates:
        if one_shot:
            go = first[k][2]
        else:
            go = redundant(S[k], c, P)[2]
            if go:
                for l in S[k]:
                    c[l] -= 1
        if go:
            state[k] = CULLED
            culled.append(k)
            if P["max_cull"] > 0 and len(culled) >= P["max_cull"]:
                break
    return dict(n_keyframes=nkf, n_candidates=len(candidates), n_redundant_initial=sum(1 for f in first if f[2]), n_culled=len(culled),
                culled_frame_id=np.array([frames[k] for k in culled], np.uint64), kf_observed=np.array([f[0] for f in first], np.int32),
                kf_redundant=np.array([f[1] for f in first], np.int32), kf_state=np.array(state, np.uint8))


def apply(keyframes, landmarks, observations, culled_frame_id, drop_orphans=1):
    """-> (keyframes, landmarks, observations, n_observations_removed, n_landmarks_removed): the three tables after the culled keyframes left,
    with every column the getters return (the landmarks' obs_offsets / obs_ids are the rows that name them, in table order)"""
    gone = set(int(f) for f in culled_frame_id)
    keep_kf = [k for k, f in enumerate(keyframes["frame_id"]) if int(f) not in gone]
    keep_ob = [i for i, f in enumerate(observations["frame_id"]) if int(f) not in gone]
    before, after, removed = {}, {}, {}
    for i, (f, l) in enumerate(zip(observations["frame_id"], observations["landmark_id"])):
        before.setdefault(int(l), []).append(i)
        if int(f) in gone:
            removed[int(l)] = removed.get(int(l), 0) + 1
        else:
            after.setdefault(int(l), []).append(i)
    keep_lm = [j for j, l in enumerate(landmarks["id"]) if not (drop_orphans and int(l) in before and int(l) not in after)]
    kfs = {}
    offs, ids = [0], []
    for k in keep_kf:
        ids.extend(keyframes["obs_ids"][keyframes["obs_offsets"][k]:keyframes["obs_offsets"][k + 1]].tolist())
        offs.append(len(ids))
    for key in ("frame_id", "stamp_ns", "R", "t"):
        kfs[key] = np.asarray(keyframes[key])[keep_kf]
    kfs["obs_offsets"] = np.array(offs, np.int64); kfs["obs_ids"] = np.array(ids, np.uint64)
    obs = {key: np.asarray(observations[key])[keep_ob] for key in observations}
    lms = {key: np.asarray(landmarks[key])[keep_lm] for key in landmarks if key not in ("obs_offsets", "obs_ids")}
    lms["observation_count"] = np.array([max(int(landmarks["observation_count"][j]) - removed.get(int(landmarks["id"][j]), 0), 0) for j in keep_lm], np.int32)
    offs, ids = [0], []
    for j in keep_lm:
        ids.extend(int(observations["id"][i]) for i in after.get(int(landmarks["id"][j]), []))
        offs.append(len(ids))
    lms["obs_offsets"] = np.array(offs, np.int64); lms["obs_ids"] = np.array(ids, np.uint64)
    return kfs, lms, obs, len(observations["frame_id"]) - len(keep_ob), len(landmarks["id"]) - len(keep_lm)


def cull(keyframes, landmarks, observations, ref_frame_id=None, protected=(), do_apply=True, **params):
    """what MappingBackend.cull_keyframes returns, and the three tables after the call -> (report, keyframes, landmarks, observations)"""
    rep = decide(keyframes, landmarks, observations, ref_frame_id, protected, **params)
    kfs, lms, obs, n_ob, n_lm = apply(keyframes, landmarks, observations, rep["culled_frame_id"], dict(DEFAULTS, **params)["drop_orphans"])
    rep["n_observations_removed"] = n_ob; rep["n_landmarks_removed"] = n_lm
    if not do_apply or rep["n_culled"] == 0:
        return rep, keyframes, landmarks, observations
    return rep, kfs, lms, obs


def rows_per_landmark(landmarks, observations):
    """per landmark of the table the number of observation rows that name it"""
    n = {}
    for l in observations["landmark_id"]:
        n[int(l)] = n.get(int(l), 0) + 1
    return np.array([n.get(int(l), 0) for l in landmarks["id"]], np.int32)
