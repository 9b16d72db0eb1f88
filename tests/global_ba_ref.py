"""Restatement of the problem dvs_backend_global_ba assembles (include/dvslam_hip.h "Global BA of the map"), over the arrays the getters
return (MappingBackend.keyframes() / landmarks() / observations(), or hand-made dicts of the same columns):
  cameras       all keyframes in table order through dvs_ba_pose_from_rt (host arithmetic), keyframe 0 fixed;
  landmarks     all rows (ascending id), float -> double, none fixed;
  observations  table order, those whose landmark id is in the landmark table, then only those of landmarks with >= 2 such rows;
  settings      the backend's intrinsics, sigma 1, Huber 1.345.
PARITY UNPINNED: the rule is the library's own."""
import numpy as np


def pose_from_rt(R, t):
    from dvslam_amd._lib import lib, check, ptr
    q = np.zeros(4); tr = np.zeros(3)
    check(lib().dvs_ba_pose_from_rt(ptr(np.ascontiguousarray(R, np.float64).reshape(9)), ptr(np.ascontiguousarray(t, np.float64).reshape(3)), ptr(q), ptr(tr)))
    return q, tr


def pose_to_rt(q, tr):
    from dvslam_amd._lib import lib, check, ptr
    R = np.zeros((3, 3)); t = np.zeros(3)
    check(lib().dvs_ba_pose_to_rt(ptr(np.ascontiguousarray(q, np.float64)), ptr(np.ascontiguousarray(tr, np.float64)), ptr(R), ptr(t)))
    return R, t


def assemble(keyframes, landmarks, observations, fx, fy, cx, cy):
    """-> (problem dict as BAProblem takes it, n_left_out, mask of the landmarks that have observations in the problem)"""
    kf_slot = {int(f): k for k, f in enumerate(keyframes["frame_id"])}
    lm_ids = [int(i) for i in landmarks["id"]]
    assert lm_ids == sorted(lm_ids)
    lm_slot = {i: k for k, i in enumerate(lm_ids)}
    rows = [(kf_slot[int(f)], lm_slot[int(l)], px) for f, l, px in zip(observations["frame_id"], observations["landmark_id"], observations["px"])
            if int(l) in lm_slot and int(f) in kf_slot]
    count = np.zeros(len(lm_ids), np.int64)
    for _, l, _ in rows:
        count[l] += 1
    rows = [r for r in rows if count[r[1]] >= 2]
    K, L = len(kf_slot), len(lm_ids)
    q = np.zeros((K, 4)); t = np.zeros((K, 3))
    for k in range(K):
        q[k], t[k] = pose_from_rt(keyframes["R"][k], keyframes["t"][k])
    pose_fixed = np.zeros(K, np.uint8); pose_fixed[0] = 1
    prob = dict(K=K, L=L, q=q, t=t, X=np.asarray(landmarks["xyz"], np.float32).astype(np.float64).reshape(L, 3),
                cam_idx=np.array([r[0] for r in rows], np.int32), lm_idx=np.array([r[1] for r in rows], np.int32),
                uv=np.array([np.asarray(r[2], np.float32).astype(np.float64) for r in rows], np.float64).reshape(-1, 2),
                pose_fixed=pose_fixed, lm_fixed=np.zeros(L, np.uint8), fx=fx, fy=fy, cx=cx, cy=cy, sigma=1.0, huber=1.345)
    return prob, len(observations["frame_id"]) - len(rows), count >= 2
