"""Reference of the tracking front end for the tests: Frontend::syncCallback (frontend.cpp:1068-1324) restated as a frame loop over a
`stages` object (tools/replay_tracking.py's HipStages / CpuStages: one host-pointer call per stage), the way replay_tracking.track()
does, with what dvs_tracker_track adds to it:
  * feature culling in std::sort's order (frontend.cpp:1201-1202: the comparator looks at the response only, ties are libstdc++'s) —
    through dvs_test_cull_order, which tests/test_tracker_cull_order.py holds against the real std::sort;
  * the 3D points of estimateCameraPose from the PREVIOUS frame's depth image (frontend.cpp:1239);
  * isKeyframe's first call returns true because has_last_keyframe_ is still false (frontend.cpp:603-606: the first frame publishes
    without asking isKeyframe), so frame 1 is a keyframe;
  * the pose arithmetic in double with explicit loops, operation for operation what csrc/tracker.hip does, so R_ / t_ compare bit for bit.
Returns one dict per frame with the fields of dvs_track_result plus `payload` and `sel`."""
import ctypes as C
import math
import numpy as np


def cull_order(hooks, response, matched, max_new=200, min_response=50.0):
    response = np.ascontiguousarray(response, np.float32); matched = np.ascontiguousarray(matched, np.uint8)
    n = len(response)
    order = np.zeros(max(n, 1), np.int32); m = C.c_int32()
    hooks.dvs_test_cull_order.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_void_p, C.POINTER(C.c_int32)]
    hooks.dvs_test_cull_order.restype = None
    hooks.dvs_test_cull_order(response.ctypes.data, matched.ctypes.data, n, max_new, min_response, order.ctypes.data, C.byref(m))
    return order[:m.value].astype(np.int64)


def rodrigues(w):
    th = math.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
    if th < 1e-15:
        return [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    k = [w[0] / th, w[1] / th, w[2] / th]
    c, s = math.cos(th), math.sin(th)
    c1 = 1.0 - c
    K = [[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]]
    return [[((c if i == j else 0.0) + c1 * (k[i] * k[j])) + s * K[i][j] for j in range(3)] for i in range(3)]


def inverse_motion(rvec, tvec):
    """frontend.cpp:937-938 and what isMotionOutlier (:549-570) looks at -> (Ri, ti, |ti|, cos of the angle BEFORE the clamp)"""
    Rr = rodrigues([float(v) for v in rvec]); tv = [float(v) for v in tvec]
    Ri = [[Rr[j][i] for j in range(3)] for i in range(3)]
    ti = [-((Ri[i][0] * tv[0] + Ri[i][1] * tv[1]) + Ri[i][2] * tv[2]) for i in range(3)]
    tn = math.sqrt((ti[0] * ti[0] + ti[1] * ti[1]) + ti[2] * ti[2])
    ca = (((Ri[0][0] + Ri[1][1]) + Ri[2][2]) - 1.0) / 2.0
    return Ri, ti, tn, ca


def pose_step(R_, t_, rvec, tvec, max_translation=0.5, max_rotation=0.2):
    """frontend.cpp:925-948 -> (updated, R_, t_): the pose composed with the inverse of PnP's motion unless that is a motion outlier"""
    Ri, ti, tn, ca = inverse_motion(rvec, tvec)
    ang = math.acos(-1.0 if ca < -1.0 else (1.0 if ca > 1.0 else ca))
    if tn > max_translation or ang > max_rotation:                             # :549-570
        return False, R_, t_
    t_ = [t_[i] + ((R_[i][0] * ti[0] + R_[i][1] * ti[1]) + R_[i][2] * ti[2]) for i in range(3)]
    R_ = [[(R_[i][0] * Ri[0][j] + R_[i][1] * Ri[1][j]) + R_[i][2] * Ri[2][j] for j in range(3)] for i in range(3)]
    return True, R_, t_


def quat_xyzw(R):
    tr1 = ((1.0 + R[0][0]) + R[1][1]) + R[2][2]
    w = math.sqrt(tr1 if tr1 > 0.0 else 0.0) / 2.0
    return [(R[2][1] - R[1][2]) / (4 * w), (R[0][2] - R[2][0]) / (4 * w), (R[1][0] - R[0][1]) / (4 * w), w]


def pts_of(kps, idx):
    return np.stack([kps["x"][idx], kps["y"][idx]], 1).astype(np.float32).reshape(-1, 2)


def _fm(stages, p1, p2, seed, fm_mode):
    if fm_mode == 1:
        return stages.fundamental_inliers(p1, p2, seed)                       # the _cv form on either side
    if stages.name == "hip":
        return stages.g.find_fundamental_ransac(p1, p2, 2.0, 0.99, 1000, seed)[1].astype(bool)
    return stages.ob.find_fundamental_ransac(p1, p2, 2.0, 0.99, 1000, seed)[1].astype(bool)


def track_ref(stages, hooks, frames, depths, f, cx, cy, fm_mode=0, pnp_mode=0, seed_base=0, to_gray=None):
    import replay_tracking as rt
    saved = rt.PNP_MODE
    rt.PNP_MODE = "cv" if pnp_mode == 1 else "own"
    try:
        return _track_ref(stages, hooks, frames, depths, f, cx, cy, fm_mode, seed_base, to_gray)
    finally:
        rt.PNP_MODE = saved


def _track_ref(stages, hooks, frames, depths, f, cx, cy, fm_mode, seed_base, to_gray):
    K4 = np.array([f, f, cx, cy])
    R_ = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    t_ = [0.0, 0.0, 0.0]
    prev_valid, has_last_kf = False, False
    prev_k = prev_d = prev_depth = None
    kf_k = kf_d = None
    since_kf, keyframe_id = 0, 0
    out = []
    for t, (img, depth) in enumerate(zip(frames, depths)):
        rows, cols = depth.shape
        gray = to_gray(img) if img.ndim == 3 else img                          # :1084
        k, d = stages.extract(gray)
        fk, fd = stages.filter_depth(k, d, depth)                              # :1100
        r = dict(frame_index=t, keyframe_id=-1, n_extracted=len(k), n_filtered=len(fk), n_matches=0, n_geometric=0, n_pnp_points=0, n_pnp_inliers=0,
                 n_backend=0, n_kf_matches=-1, n_kf_geometric=-1, first_frame=0, tracking_reset=0, fm_skipped=0, pnp_skipped=0, pnp_failed=0,
                 motion_outlier=0, pose_updated=0, is_keyframe=0, kf_criterion=0, rvec=np.zeros(3), tvec=np.zeros(3), payload=None, sel=np.zeros(0, np.int64))
        publish = False
        if not prev_valid:                                                     # :1278-1312
            r["first_frame"] = 1
            bk, bd = fk, fd
            r["sel"] = np.arange(len(fk), dtype=np.int64)
            publish = True; r["kf_criterion"] = 1
        elif len(fk) == 0 or len(prev_k) == 0:                                 # :1107-1117
            r["tracking_reset"] = 1
            r["R"] = np.array(R_); r["t"] = np.array(t_)
            prev_k, prev_d, prev_depth = fk, fd, depth
            out.append(r)
            continue
        else:
            idx, dist = stages.match(fd, prev_d)                               # :1123
            q = np.nonzero(dist < 50)[0]; tr = idx[q]                          # :1126-1132
            r["n_matches"] = len(q)
            if len(q) >= 8:                                                    # :1136-1153
                m = _fm(stages, pts_of(prev_k, tr), pts_of(fk, q), seed_base + 2 * t, fm_mode)
                q, tr = q[m], tr[m]
            else:
                r["fm_skipped"] = 1
            r["n_geometric"] = len(q)
            matched = np.zeros(len(fk), np.uint8); matched[q] = 1              # :1171-1219
            sel = np.concatenate([q.astype(np.int64), cull_order(hooks, fk["response"], matched)])
            bk, bd = fk[sel], fd[sel]
            r["sel"] = sel
            do_pnp = False
            if len(q) >= 5:                                                    # :1237, :859-892 with prev_frame_depth_
                pp = pts_of(prev_k, tr); cp = pts_of(fk, q)
                xi = np.floor(pp[:, 0].astype(np.float64) + 0.5).astype(np.int64); yi = np.floor(pp[:, 1].astype(np.float64) + 0.5).astype(np.int64)
                inb = (xi >= 0) & (yi >= 0) & (xi < cols) & (yi < rows)
                dp = np.zeros(len(pp), np.float32)
                dp[inb] = prev_depth[yi[inb], xi[inb]].astype(np.float32) * np.float32(0.001)
                ok = inb & ~((dp <= np.float32(0.3)) | (dp > np.float32(3.0)))
                obj = np.stack([(pp[:, 0] - np.float32(cx)) * dp / np.float32(f), (pp[:, 1] - np.float32(cy)) * dp / np.float32(f), dp], 1)[ok]
                img2 = cp[ok]
                r["n_pnp_points"] = len(obj)
                do_pnp = len(obj) >= 6                                         # :899
            if not do_pnp:
                r["pnp_skipped"] = 1
            else:
                good, rvec, tvec, nin = stages.pnp(obj, img2, K4, seed=seed_base + 2 * t + 1)
                if good:
                    r["rvec"], r["tvec"] = np.array(rvec), np.array(tvec)
                    r["n_pnp_inliers"] = nin
                    updated, R_, t_ = pose_step(R_, t_, rvec, tvec)
                    r["pose_updated" if updated else "motion_outlier"] = 1
                else:
                    r["pnp_failed"] = 1
                    if rt_pnp_is_cv() and rvec is not None:
                        r["rvec"], r["tvec"] = np.array(rvec), np.array(tvec)   # the RANSAC stage's pose when only the refit failed
            if not has_last_kf:                                                # :603-606
                has_last_kf = True
                publish = True; r["kf_criterion"] = 2
            else:
                crit = False
                if len(kf_d) and len(bd):                                      # :611-651
                    ki, kd = stages.match(bd, kf_d)
                    kq = np.nonzero(kd < 50)[0]; ktr = ki[kq]
                    r["n_kf_matches"] = len(kq)
                    if len(kq) >= 8:
                        km = _fm(stages, pts_of(kf_k, ktr), pts_of(bk, kq), seed_base + 2 * t + 1000003, fm_mode)
                        kq = kq[km]
                    r["n_kf_geometric"] = len(kq)
                    crit = len(kq) < 150
                if crit or since_kf > 30:                                      # :655-660
                    r["kf_criterion"] = (4 if crit else 0) | (8 if since_kf > 30 else 0)
                    since_kf = 0; publish = True
                else:
                    since_kf += 1
        r["n_backend"] = len(bk)
        r["R"] = np.array(R_); r["t"] = np.array(t_)
        if publish:                                                            # :699-790
            r["is_keyframe"] = 1; r["keyframe_id"] = keyframe_id
            r["payload"] = stages.publish(bk, bd, depth, f, f, cx, cy, np.array(R_), np.array(t_), stamp=(t, 0), frame_id="camera_link",
                                          keyframe_id=keyframe_id, q_xyzw=quat_xyzw(R_))
            keyframe_id += 1
            kf_k, kf_d = bk, bd
        prev_k, prev_d, prev_depth, prev_valid = fk, fd, depth, True
        out.append(r)
    return out


def rt_pnp_is_cv():
    import replay_tracking as rt
    return rt.PNP_MODE == "cv"


INT_FIELDS = ("frame_index", "keyframe_id", "n_extracted", "n_filtered", "n_matches", "n_geometric", "n_pnp_points", "n_pnp_inliers", "n_backend",
              "n_kf_matches", "n_kf_geometric", "first_frame", "tracking_reset", "fm_skipped", "pnp_skipped", "pnp_failed", "motion_outlier",
              "pose_updated", "is_keyframe", "kf_criterion")


def run_tracker(tr, frames, depths):
    """the same sequence through a dvslam_amd.Tracker -> the same list of dicts"""
    out = []
    for t, (img, depth) in enumerate(zip(frames, depths)):
        r, payload = tr.track(img, depth, (t, 0))
        r["payload"] = payload
        r["sel"] = tr.backend_features()[2].astype(np.int64)
        out.append(r)
    return out


def first_difference(a, b, poses_bitwise=True):
    """None if the two runs agree in every count, flag, selection, rvec / tvec, payload (and R_ / t_ bit for bit), else a description"""
    if len(a) != len(b):
        return f"{len(a)} frames against {len(b)}"
    for t, (x, y) in enumerate(zip(a, b)):
        for k in INT_FIELDS:
            if int(x[k]) != int(y[k]):
                return f"frame {t}: {k} {x[k]} != {y[k]}"
        if not np.array_equal(x["sel"], y["sel"]):
            return f"frame {t}: culled selection differs ({len(x['sel'])} / {len(y['sel'])} rows)"
        for k in ("rvec", "tvec") + (("R", "t") if poses_bitwise else ()):
            if np.asarray(x[k], np.float64).tobytes() != np.asarray(y[k], np.float64).tobytes():
                return f"frame {t}: {k} differs by {np.abs(np.asarray(x[k]) - np.asarray(y[k])).max():.3e}"
        if x["payload"] != y["payload"]:
            return f"frame {t}: CDR payload differs"
    return None
