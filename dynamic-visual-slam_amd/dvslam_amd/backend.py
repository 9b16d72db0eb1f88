"""ctypes mirror of the mapping backend (include/dvslam_hip.h, dvs_backend_*): Backend::syncCallback, the BA window, updateOptimizedResults
and pruneLandmarks (backend.cpp) as one handle that keeps the landmark and observation tables on the device; one call per keyframe."""
import ctypes as C
import numpy as np
from ._lib import lib, check, ptr, DvsError, KeyframeHeader, PgoParams, PgoSummary, BaGlobalParams, BaGlobalSummary, BaSummary

MAX_FILTERED = 16


class BackendParams(C.Structure):
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("max_descriptor_distance", C.c_double),
                ("max_reprojection_distance", C.c_double), ("window", C.c_int32), ("prune_min_observations", C.c_int32),
                ("prune_max_age_sec", C.c_double), ("n_filtered", C.c_int32), ("filtered_class_ids", C.c_int32 * MAX_FILTERED),
                ("initial_capacity", C.c_int32)]


class Detection(C.Structure):
    _fields_ = [("cx", C.c_double), ("cy", C.c_double), ("w", C.c_double), ("h", C.c_double), ("class_id", C.c_int32), ("reserved", C.c_int32)]


class BackendResult(C.Structure):
    _fields_ = [("n_kept", C.c_int32), ("n_filtered", C.c_int32), ("n_associated", C.c_int32), ("n_created", C.c_int32), ("n_moved", C.c_int32),
                ("reserved", C.c_int32), ("first_observation_id", C.c_int64), ("first_landmark_id", C.c_int64)]
    FIELDS = ("n_kept", "n_filtered", "n_associated", "n_created", "n_moved", "first_observation_id", "first_landmark_id")

    def as_dict(self):
        return {k: int(getattr(self, k)) for k in self.FIELDS}


class BackendCount(C.Structure):
    _fields_ = [(k, C.c_int64) for k in ("n_keyframes", "n_observations", "n_landmarks", "next_observation_id", "next_landmark_id")]


class FuseParams(C.Structure):
    """dvs_fuse_params (fill it with dvs_fuse_default_params)"""
    _fields_ = [("max_descriptor_distance", C.c_double), ("max_reprojection_distance", C.c_double), ("fuse_neighbours", C.c_int32), ("reserved", C.c_int32)]


class FuseResult(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("n_sources", "n_targets", "n_proposals", "n_fused")]


class CloseLoopResult(C.Structure):
    _fields_ = [("summary", PgoSummary), ("n_nodes", C.c_int32), ("n_edges", C.c_int32), ("n_landmarks_moved", C.c_int32), ("reserved", C.c_int32),
                ("fuse", FuseResult)]


class GlobalBaResult(C.Structure):
    """dvs_backend_gba_result"""
    _fields_ = [("summary", BaGlobalSummary), ("n_cameras", C.c_int32), ("n_landmarks", C.c_int32), ("n_observations", C.c_int32), ("n_left_out", C.c_int32)]


class CovisParams(C.Structure):
    """dvs_covis_params (fill it with dvs_covis_default_params)"""
    _fields_ = [("min_weight", C.c_int32), ("max_neighbours", C.c_int32), ("max_fixed", C.c_int32), ("ba_max_iterations", C.c_int32)]


class LocalBaResult(C.Structure):
    """dvs_backend_lba_result"""
    _fields_ = [("summary", BaSummary), ("n_cameras", C.c_int32), ("n_fixed", C.c_int32), ("n_landmarks", C.c_int32), ("n_observations", C.c_int32),
                ("n_left_out", C.c_int32), ("n_dropped", C.c_int32)]


class CullParams(C.Structure):
    """dvs_cull_params (fill it with dvs_cull_default_params)"""
    _fields_ = [(k, C.c_int32) for k in ("min_observers", "redundancy_percent", "min_weight", "local", "keep_recent", "max_cull", "drop_orphans", "reserved")]


class CullResult(C.Structure):
    """dvs_cull_result"""
    _fields_ = [(k, C.c_int32) for k in ("n_keyframes", "n_candidates", "n_redundant_initial", "n_culled", "n_observations_removed", "n_landmarks_removed")] + \
               [("reserved", C.c_int32 * 2)]


class LmRefreshParams(C.Structure):
    """dvs_lm_refresh_params (fill it with dvs_lm_refresh_default_params)"""
    _fields_ = [("update_descriptors", C.c_int32), ("min_views", C.c_int32), ("use_scope", C.c_int32), ("reserved", C.c_int32), ("scope_frame_id", C.c_uint64)]


class LmRefreshResult(C.Structure):
    """dvs_lm_refresh_result"""
    _fields_ = [(k, C.c_int32) for k in ("n_in_scope", "n_changed", "n_without_views", "max_views")]


class LmCullParams(C.Structure):
    """dvs_lm_cull_params (fill it with dvs_lm_cull_default_params)"""
    _fields_ = [(k, C.c_int32) for k in ("found_ratio_pct", "min_visible", "weak_age_kf", "weak_max_views")]


class LmCullResult(C.Structure):
    """dvs_lm_cull_result"""
    _fields_ = [(k, C.c_int32) for k in ("n_landmarks", "n_by_ratio", "n_weak", "n_landmarks_removed", "n_observations_removed", "n_keyframes_touched")] + \
               [("reserved", C.c_int32 * 2)]


class MapTrackGates(C.Structure):
    """dvs_maptrack_gates (fill it with dvs_mapgate_default_gates)"""
    _fields_ = [("cos_min", C.c_double), ("range_factor", C.c_double)]


def _bind(L):
    vp, i32, i64, sz = C.c_void_p, C.c_int32, C.c_int64, C.c_size_t
    pi32, pi64 = C.POINTER(i32), C.POINTER(i64)
    L.dvs_backend_default_params.argtypes = [C.POINTER(BackendParams)]; L.dvs_backend_default_params.restype = None
    L.dvs_backend_create.argtypes = [C.POINTER(BackendParams), i32, C.POINTER(vp)]
    L.dvs_backend_destroy.argtypes = [vp]; L.dvs_backend_destroy.restype = None
    L.dvs_backend_reset.argtypes = [vp]
    L.dvs_backend_add_keyframe.argtypes = [vp, C.POINTER(KeyframeHeader), i32, vp, vp, vp, vp, i32, C.POINTER(BackendResult)]
    L.dvs_backend_add_keyframe_cdr.argtypes = [vp, vp, sz, vp, i32, C.POINTER(BackendResult)]
    L.dvs_backend_counts.argtypes = [vp, C.POINTER(BackendCount)]
    L.dvs_backend_get_window.argtypes = [vp, i32, i32, i32, vp, vp, vp, pi32, vp, vp, vp, vp, vp, pi32, vp, vp, vp, pi32]
    L.dvs_backend_apply_optimized.argtypes = [vp, i32, vp, vp, vp, i32, vp, vp, vp]
    L.dvs_backend_prune.argtypes = [vp, i32, C.c_uint32, pi32, pi32]
    L.dvs_backend_get_landmarks.argtypes = [vp, i32, i64, vp, vp, vp, vp, vp, vp, vp, vp, pi32, pi64]
    L.dvs_backend_get_observations.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, pi32]
    L.dvs_backend_get_keyframes.argtypes = [vp, i32, i64, vp, vp, vp, vp, vp, vp, pi32, pi64]
    dbl, u64 = C.c_double, C.c_uint64
    L.dvs_fuse_default_params.argtypes = [C.POINTER(FuseParams)]
    L.dvs_backend_get_anchors.argtypes = [vp, i32, vp, vp, pi32]
    L.dvs_backend_build_pose_graph.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, dbl, dbl, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, pi32, pi32]
    L.dvs_backend_close_loop.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp, vp, dbl, dbl, C.POINTER(PgoParams), C.POINTER(FuseParams), C.POINTER(CloseLoopResult)]
    L.dvs_backend_fuse.argtypes = [vp, u64, vp, i32, C.POINTER(FuseParams), i32, C.POINTER(FuseResult), i32, vp, vp, vp, pi32]
    L.dvs_backend_global_ba.argtypes = [vp, vp, C.POINTER(BaGlobalParams), C.POINTER(GlobalBaResult)]
    pcv = C.POINTER(CovisParams)
    L.dvs_covis_default_params.argtypes = [pcv]; L.dvs_covis_default_params.restype = None
    L.dvs_backend_covisibility.argtypes = [vp, i32, i32, i64, vp, vp, vp, vp, pi32, pi64]
    L.dvs_backend_get_local_window.argtypes = [vp, u64, pcv, i32, i32, i32, vp, vp, vp, vp, vp, pi32, vp, vp, vp, vp, vp, pi32, vp, vp, vp, pi32, pi32]
    L.dvs_backend_local_ba.argtypes = [vp, vp, u64, pcv, C.POINTER(LocalBaResult)]
    L.dvs_cull_default_params.argtypes = [C.POINTER(CullParams)]; L.dvs_cull_default_params.restype = None
    L.dvs_backend_cull_keyframes.argtypes = [vp, u64, C.POINTER(CullParams), vp, i32, i32, C.POINTER(CullResult), i32, vp, vp, vp, vp, pi32]
    L.dvs_lm_refresh_default_params.argtypes = [C.POINTER(LmRefreshParams)]; L.dvs_lm_refresh_default_params.restype = None
    L.dvs_mapgate_default_gates.argtypes = [C.POINTER(MapTrackGates)]; L.dvs_mapgate_default_gates.restype = None
    L.dvs_backend_refresh_landmarks.argtypes = [vp, C.POINTER(LmRefreshParams), C.POINTER(LmRefreshResult)]
    L.dvs_backend_get_landmark_geometry.argtypes = [vp, i32, vp, vp, vp, vp, vp, pi32]
    L.dvs_backend_track_frame_gated.argtypes = [vp, vp, C.POINTER(MapTrackGates), vp, vp, i32, vp, vp, vp]
    L.dvs_lm_cull_default_params.argtypes = [C.POINTER(LmCullParams)]; L.dvs_lm_cull_default_params.restype = None
    L.dvs_backend_set_tracking_stats.argtypes = [vp, i32]
    L.dvs_backend_cull_landmarks.argtypes = [vp, C.POINTER(LmCullParams), i32, C.POINTER(LmCullResult), i32, vp, vp, pi32]
    L.dvs_backend_get_landmark_stats.argtypes = [vp, i32, vp, vp, vp, vp, vp, pi32, pi64]
    L.dvs_backend_set_landmark_stats.argtypes = [vp, i32, vp, vp, vp]
    L.dvs_backend_clear_landmark_stats.argtypes = [vp]
    return L


def fuse_params(**kw):
    """dvs_fuse_default_params with field overrides"""
    p = FuseParams()
    check(_bind(lib()).dvs_fuse_default_params(C.byref(p)))
    for k, v in kw.items():
        if k not in dict(FuseParams._fields_) or k == "reserved":
            raise TypeError(f"unknown parameter {k}")
        setattr(p, k, v)
    return p


def covis_params(**kw):
    """dvs_covis_default_params with field overrides"""
    p = CovisParams()
    _bind(lib()).dvs_covis_default_params(C.byref(p))
    for k, v in kw.items():
        if k not in dict(CovisParams._fields_):
            raise TypeError(f"unknown parameter {k}")
        setattr(p, k, v)
    return p


def cull_params(**kw):
    """dvs_cull_default_params with field overrides"""
    p = CullParams()
    _bind(lib()).dvs_cull_default_params(C.byref(p))
    for k, v in kw.items():
        if k not in dict(CullParams._fields_) or k == "reserved":
            raise TypeError(f"unknown parameter {k}")
        setattr(p, k, v)
    return p


def lm_cull_params(**kw):
    """dvs_lm_cull_default_params with field overrides"""
    p = LmCullParams()
    _bind(lib()).dvs_lm_cull_default_params(C.byref(p))
    for k, v in kw.items():
        if k not in dict(LmCullParams._fields_) or k == "reserved":
            raise TypeError(f"unknown parameter {k}")
        setattr(p, k, int(v))
    return p


def lm_refresh_params(scope_frame_id=None, **kw):
    """dvs_lm_refresh_default_params with field overrides; scope_frame_id None: the whole table"""
    p = LmRefreshParams()
    _bind(lib()).dvs_lm_refresh_default_params(C.byref(p))
    for k, v in kw.items():
        if k not in ("update_descriptors", "min_views"):
            raise TypeError(f"unknown parameter {k}")
        setattr(p, k, int(v))
    if scope_frame_id is not None:
        p.use_scope, p.scope_frame_id = 1, int(scope_frame_id)
    return p


def maptrack_gates(**kw):
    """dvs_mapgate_default_gates with field overrides"""
    g = MapTrackGates()
    _bind(lib()).dvs_mapgate_default_gates(C.byref(g))
    for k, v in kw.items():
        if k not in dict(MapTrackGates._fields_):
            raise TypeError(f"unknown parameter {k}")
        setattr(g, k, float(v))
    return g


def _loop_arrays(loops):
    """[(query frame id, entry frame id, rvec, tvec, w_rot, w_trans)] -> the six arrays of the C-ABI"""
    q = np.array([l[0] for l in loops], np.uint64); e = np.array([l[1] for l in loops], np.uint64)
    rv = np.array([np.asarray(l[2], np.float64).reshape(3) for l in loops], np.float64).reshape(-1, 3)
    tv = np.array([np.asarray(l[3], np.float64).reshape(3) for l in loops], np.float64).reshape(-1, 3)
    wr = np.array([l[4] for l in loops], np.float64); wt = np.array([l[5] for l in loops], np.float64)
    return q, e, rv, tv, wr, wt


def default_params(fx=0.0, fy=0.0, cx=0.0, cy=0.0, filtered_class_ids=(), **kw):
    """dvs_backend_default_params (the reference's constants) with the intrinsics, the filtered class ids and any field overrides"""
    p = BackendParams()
    _bind(lib()).dvs_backend_default_params(C.byref(p))
    p.fx, p.fy, p.cx, p.cy = fx, fy, cx, cy
    ids = [int(c) for c in filtered_class_ids]
    if len(ids) > MAX_FILTERED:
        raise ValueError(f"at most {MAX_FILTERED} filtered classes")
    p.n_filtered = len(ids)
    for k, c in enumerate(ids):
        p.filtered_class_ids[k] = c
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


class MappingBackend:
    """mb = MappingBackend(fx, fy, cx, cy, filtered=("person",)); r = mb.add_keyframe_cdr(payload, [(cx, cy, w, h, "chair"), ...])

    Class names are interned: 0 is "unlabeled", every other name gets the next id the first time it is seen."""

    def __init__(self, fx, fy, cx, cy, filtered=("person",), device=0, **kw):
        self._L = _bind(lib())
        self._h = None
        self._ba = None
        self._gba = None
        self.fx, self.fy, self.cx, self.cy, self.device = fx, fy, cx, cy, device
        self.class_names = ["unlabeled"]
        self._class_id = {"unlabeled": 0}
        self.params = default_params(fx, fy, cx, cy, [self.intern(c) for c in filtered], **kw)
        h = C.c_void_p()
        check(self._L.dvs_backend_create(C.byref(self.params), device, C.byref(h)))
        self._h = h

    def intern(self, name):
        if name not in self._class_id:
            self._class_id[name] = len(self.class_names); self.class_names.append(name)
        return self._class_id[name]

    def _detections(self, detections):
        arr = (Detection * max(len(detections), 1))()
        for k, (cx, cy, w, h, name) in enumerate(detections):
            arr[k] = Detection(float(cx), float(cy), float(w), float(h), self.intern(name) if isinstance(name, str) else int(name), 0)
        return arr, len(detections)

    def add_keyframe(self, frame_id, stamp, translation, rotation_xyzw, landmark_xyz, obs_pixels, obs_desc, detections=()):
        """syncCallback on flat arrays (landmark_xyz (n, 3) and obs_pixels (n, 2) float64, obs_desc (n, 32) uint8) -> result dict"""
        from .glue import FrontendGlue
        hdr = FrontendGlue._header(stamp, "camera_link", frame_id, translation, rotation_xyzw)
        xyz = np.ascontiguousarray(landmark_xyz, np.float64).reshape(-1, 3); px = np.ascontiguousarray(obs_pixels, np.float64).reshape(-1, 2)
        desc = np.ascontiguousarray(obs_desc, np.uint8).reshape(-1, 32)
        if not len(xyz) == len(px) == len(desc):
            raise ValueError("landmark_xyz, obs_pixels and obs_desc must have one row per observation")
        det, nd = self._detections(detections)
        r = BackendResult()
        check(self._L.dvs_backend_add_keyframe(self._h, C.byref(hdr), len(px), ptr(xyz), ptr(px), ptr(desc), C.cast(det, C.c_void_p), nd, C.byref(r)))
        return r.as_dict()

    def add_keyframe_cdr(self, payload, detections=()):
        """the same on the Keyframe.msg CDR payload of publish_keyframe / Tracker.track"""
        buf = np.frombuffer(payload, np.uint8)
        det, nd = self._detections(detections)
        r = BackendResult()
        check(self._L.dvs_backend_add_keyframe_cdr(self._h, buf.ctypes.data, len(buf), C.cast(det, C.c_void_p), nd, C.byref(r)))
        return r.as_dict()

    def counts(self):
        c = BackendCount()
        check(self._L.dvs_backend_counts(self._h, C.byref(c)))
        return {k: int(getattr(c, k)) for k, _ in BackendCount._fields_}

    def window(self):
        """the BA window: dict of keyframes (frame_id, R, t), observations (px, landmark_id, class_id, frame_id, lm_index) and landmarks
        (id, class_id, xyz) as arrays"""
        c = self.counts()
        ck, co, cl = max(int(self.params.window), 1), max(c["n_observations"], 1), max(c["n_landmarks"], 1)
        kid = np.zeros(ck, np.uint64); R = np.zeros((ck, 3, 3)); t = np.zeros((ck, 3))
        px = np.zeros((co, 2), np.float32); olm = np.zeros(co, np.uint64); ocl = np.zeros(co, np.int32); ofr = np.zeros(co, np.uint64); oix = np.zeros(co, np.int32)
        lid = np.zeros(cl, np.uint64); lcl = np.zeros(cl, np.int32); xyz = np.zeros((cl, 3), np.float32)
        nk, no, nl = C.c_int32(), C.c_int32(), C.c_int32()
        check(self._L.dvs_backend_get_window(self._h, ck, co, cl, ptr(kid), ptr(R), ptr(t), C.byref(nk), ptr(px), ptr(olm), ptr(ocl), ptr(ofr), ptr(oix), C.byref(no),
                                             ptr(lid), ptr(lcl), ptr(xyz), C.byref(nl)))
        nk, no, nl = nk.value, no.value, nl.value
        return dict(kf_frame_id=kid[:nk], kf_R=R[:nk], kf_t=t[:nk], obs_px=px[:no], obs_landmark_id=olm[:no], obs_class=ocl[:no], obs_frame_id=ofr[:no],
                    obs_lm_index=oix[:no], lm_id=lid[:nl], lm_class=lcl[:nl], lm_xyz=xyz[:nl])

    def apply_optimized(self, poses, landmarks):
        """updateOptimizedResults: poses {frame_id: (R, t)}, landmarks {(id, class_id): xyz}"""
        fid = np.array(list(poses.keys()), np.uint64)
        R = np.array([np.asarray(p[0], np.float64).reshape(9) for p in poses.values()], np.float64).reshape(-1, 9)
        t = np.array([np.asarray(p[1], np.float64).reshape(3) for p in poses.values()], np.float64).reshape(-1, 3)
        lid = np.array([k[0] for k in landmarks.keys()], np.uint64); lcl = np.array([k[1] for k in landmarks.keys()], np.int32)
        xyz = np.array([np.asarray(v, np.float64).reshape(3) for v in landmarks.values()], np.float64).reshape(-1, 3)
        check(self._L.dvs_backend_apply_optimized(self._h, len(fid), ptr(fid), ptr(R), ptr(t), len(lid), ptr(lid), ptr(lcl), ptr(xyz)))

    def prune(self, now):
        """pruneLandmarks at now = (sec, nanosec) -> (removed landmarks, removed observations)"""
        a, b = C.c_int32(), C.c_int32()
        check(self._L.dvs_backend_prune(self._h, int(now[0]), int(now[1]), C.byref(a), C.byref(b)))
        return a.value, b.value

    def bundle_adjust(self, now, max_iterations=20):
        """bundleAdjustmentCallback: window -> SlidingWindowBA.optimize(..., 20) -> apply on success -> prune.  Returns (result dict, pruned)"""
        from .ba import SlidingWindowBA
        w = self.window()
        kfs = [(int(f), w["kf_R"][k], w["kf_t"][k]) for k, f in enumerate(w["kf_frame_id"])]
        lms = [(int(i), int(c), w["lm_xyz"][k].astype(np.float64), False) for k, (i, c) in enumerate(zip(w["lm_id"], w["lm_class"]))]
        obs = [((float(p[0]), float(p[1])), int(l), int(c), int(f)) for p, l, c, f in zip(w["obs_px"], w["obs_landmark_id"], w["obs_class"], w["obs_frame_id"])]
        if self._ba is None:
            self._ba = SlidingWindowBA(self.fx, self.fy, self.cx, self.cy, device=self.device)
        res = self._ba.optimize(kfs, lms, obs, max_iterations)
        if res["success"]:
            self.apply_optimized(res["optimized_poses"], res["optimized_landmarks"])
        return res, self.prune(now)

    def landmarks(self):
        c = self.counts()
        n, m = max(c["n_landmarks"], 1), max(c["n_observations"], 1)
        lid = np.zeros(n, np.uint64); cl = np.zeros(n, np.int32); xyz = np.zeros((n, 3), np.float32); desc = np.zeros((n, 32), np.uint8)
        cnt = np.zeros(n, np.int32); seen = np.zeros(n, np.int64); offs = np.zeros(n + 1, np.int64); oid = np.zeros(m, np.uint64)
        nn, nm = C.c_int32(), C.c_int64()
        check(self._L.dvs_backend_get_landmarks(self._h, n, m, ptr(lid), ptr(cl), ptr(xyz), ptr(desc), ptr(cnt), ptr(seen), ptr(offs), ptr(oid), C.byref(nn), C.byref(nm)))
        n = nn.value
        return dict(id=lid[:n], class_id=cl[:n], xyz=xyz[:n], desc=desc[:n], observation_count=cnt[:n], last_seen_ns=seen[:n], obs_offsets=offs[:n + 1],
                    obs_ids=oid[:nm.value])

    def observations(self):
        n = max(self.counts()["n_observations"], 1)
        oid = np.zeros(n, np.uint64); fr = np.zeros(n, np.uint64); px = np.zeros((n, 2), np.float32); desc = np.zeros((n, 32), np.uint8)
        cl = np.zeros(n, np.int32); lm = np.zeros(n, np.uint64); nn = C.c_int32()
        check(self._L.dvs_backend_get_observations(self._h, n, ptr(oid), ptr(fr), ptr(px), ptr(desc), ptr(cl), ptr(lm), C.byref(nn)))
        n = nn.value
        return dict(id=oid[:n], frame_id=fr[:n], px=px[:n], desc=desc[:n], class_id=cl[:n], landmark_id=lm[:n])

    def keyframes(self):
        c = self.counts()
        n, m = max(c["n_keyframes"], 1), max(c["n_observations"], 1)
        fid = np.zeros(n, np.uint64); st = np.zeros(n, np.int64); R = np.zeros((n, 3, 3)); t = np.zeros((n, 3)); offs = np.zeros(n + 1, np.int64)
        oid = np.zeros(m, np.uint64); nn, nm = C.c_int32(), C.c_int64()
        check(self._L.dvs_backend_get_keyframes(self._h, n, m, ptr(fid), ptr(st), ptr(R), ptr(t), ptr(offs), ptr(oid), C.byref(nn), C.byref(nm)))
        n = nn.value
        return dict(frame_id=fid[:n], stamp_ns=st[:n], R=R[:n], t=t[:n], obs_offsets=offs[:n + 1], obs_ids=oid[:nm.value])

    # ---- loop closing on the map (include/dvslam_hip.h "Loop closing on the map")
    def anchors(self):
        """(landmark ids ascending, keyframe index of each landmark's lowest-id observation or -1)"""
        n = max(self.counts()["n_landmarks"], 1)
        lid = np.zeros(n, np.uint64); anc = np.zeros(n, np.int32); nn = C.c_int32()
        check(self._L.dvs_backend_get_anchors(self._h, n, ptr(lid), ptr(anc), C.byref(nn)))
        return lid[:nn.value], anc[:nn.value]

    def build_pose_graph(self, loops, odo_w):
        """loops: [(query frame id, entry frame id, rvec, tvec, w_rot, w_trans)], odo_w = (w_rot, w_trans) -> dict of the arrays
        PoseGraph.set_nodes / set_edges take: R, t, fixed, ei, ej, rvec, tvec, w_rot, w_trans"""
        q, e, rv, tv, wr, wt = _loop_arrays(loops)
        cn = max(self.counts()["n_keyframes"], 1); ce = cn + len(loops)
        R = np.zeros((cn, 3, 3)); t = np.zeros((cn, 3)); fixed = np.zeros(cn, np.uint8); ei = np.zeros(ce, np.int32); ej = np.zeros(ce, np.int32)
        rvec = np.zeros((ce, 3)); tvec = np.zeros((ce, 3)); w_rot = np.zeros(ce); w_trans = np.zeros(ce); nn, ne = C.c_int32(), C.c_int32()
        check(self._L.dvs_backend_build_pose_graph(self._h, len(loops), ptr(q), ptr(e), ptr(rv), ptr(tv), ptr(wr), ptr(wt), float(odo_w[0]), float(odo_w[1]), cn, ce,
                                                   ptr(R), ptr(t), ptr(fixed), ptr(ei), ptr(ej), ptr(rvec), ptr(tvec), ptr(w_rot), ptr(w_trans), C.byref(nn), C.byref(ne)))
        nn, ne = nn.value, ne.value
        return dict(R=R[:nn], t=t[:nn], fixed=fixed[:nn], ei=ei[:ne], ej=ej[:ne], rvec=rvec[:ne], tvec=tvec[:ne], w_rot=w_rot[:ne], w_trans=w_trans[:ne])

    def fuse(self, query, entries, apply=True, pairs=True, **params):
        """dvs_backend_fuse: landmarks seen from the entry keyframes merged into the duplicates the query keyframe created -> dict of the four
        counts and, unless pairs=False (the pair list then stays on the device), pairs = (survivor ids, removed ids, reprojection errors) in
        ascending removed id"""
        p = fuse_params(**params)
        ent = np.array([int(f) for f in entries], np.uint64)
        cap = max(self.counts()["n_landmarks"], 1) if pairs else 0
        sv = np.zeros(cap, np.uint64); rm = np.zeros(cap, np.uint64); err = np.zeros(cap, np.float64); r = FuseResult(); n = C.c_int32()
        check(self._L.dvs_backend_fuse(self._h, int(query), ptr(ent), len(ent), C.byref(p), 1 if apply else 0, C.byref(r), cap, ptr(sv) if pairs else None,
                                       ptr(rm) if pairs else None, ptr(err) if pairs else None, C.byref(n)))
        out = {k: int(getattr(r, k)) for k, _ in FuseResult._fields_}
        if pairs:
            out["pairs"] = (sv[:n.value], rm[:n.value], err[:n.value])
        return out

    def close_loop(self, pose_graph, loops, odo_w, pgo_params=None, fuse=None):
        """dvs_backend_close_loop on a dvslam_amd.PoseGraph of the same device: pgo_params / fuse are dicts of field overrides (fuse=None: no
        fusion, fuse={}: the defaults) -> dict(summary=PgoSummary, n_nodes, n_edges, n_landmarks_moved, n_sources, n_targets, n_proposals, n_fused)"""
        q, e, rv, tv, wr, wt = _loop_arrays(loops)
        pp = None
        if pgo_params is not None:
            pp = PgoParams()
            check(self._L.dvs_pgo_default_params(C.byref(pp)))
            for k, v in pgo_params.items():
                if k not in dict(PgoParams._fields_):
                    raise TypeError(f"unknown parameter {k}")
                setattr(pp, k, v)
        fp = fuse_params(**fuse) if fuse is not None else None
        r = CloseLoopResult()
        check(self._L.dvs_backend_close_loop(self._h, pose_graph._h, len(loops), ptr(q), ptr(e), ptr(rv), ptr(tv), ptr(wr), ptr(wt), float(odo_w[0]), float(odo_w[1]),
                                             C.byref(pp) if pp is not None else None, C.byref(fp) if fp is not None else None, C.byref(r)))
        out = dict(summary=r.summary, n_nodes=r.n_nodes, n_edges=r.n_edges, n_landmarks_moved=r.n_landmarks_moved)
        out.update({k: int(getattr(r.fuse, k)) for k, _ in FuseResult._fields_})
        return out

    def global_bundle_adjust(self, ba=None, **params):
        """dvs_backend_global_ba: every keyframe and landmark of the map refined by BAProblem.solve_global (the step after close_loop), on
        `ba` (a dvslam_amd.BAProblem of the same device; None: a handle this object creates once and keeps).  params: the fields of
        dvs_ba_global_params.  The map changes only if the solve converged (summary.ba.termination == 0).
        -> dict(summary=dvs_ba_global_summary, n_cameras, n_landmarks, n_observations, n_left_out)"""
        from .ba import BAProblem
        if ba is None:
            if self._gba is None:
                self._gba = BAProblem.empty(self.device)
            ba = self._gba
        p = BaGlobalParams()
        check(self._L.dvs_ba_default_global_params(C.byref(p)))
        for k, v in params.items():
            if k not in dict(BaGlobalParams._fields_):
                raise TypeError(f"unknown parameter {k}")
            setattr(p, k, v)
        r = GlobalBaResult()
        check(self._L.dvs_backend_global_ba(self._h, ba._h, C.byref(p), C.byref(r)))
        return dict(summary=r.summary, n_cameras=r.n_cameras, n_landmarks=r.n_landmarks, n_observations=r.n_observations, n_left_out=r.n_left_out)

    def track_frame(self, map_tracker, d_kps, d_desc, n_kp, R, t):
        """dvs_backend_track_frame: a frame's keypoints and descriptors (device pointers or DeviceBuffers) against the landmark table as it
        stands, prior camera-to-world pose (R, t) -> map_track result dict; the map is not modified"""
        from . import map_track as M
        M._bind(self._L)
        R = np.ascontiguousarray(R, np.float64).reshape(9); t = np.ascontiguousarray(t, np.float64).reshape(3)
        r = M.MapTrackResult()
        check(self._L.dvs_backend_track_frame(self._h, map_tracker.handle, M._raw(d_kps), M._raw(d_desc), int(n_kp), ptr(R), ptr(t), C.byref(r)))
        return r.as_dict()

    def relocalize_frame(self, relocalizer, map_tracker, d_kps, d_desc, n_kp):
        """dvs_backend_relocalize_frame: a frame's keypoints and descriptors (device pointers or DeviceBuffers) against the landmark table as
        it stands, no prior pose -> reloc result dict; the map is not modified"""
        from . import map_track as M, reloc as RL
        RL._bind(self._L)
        r = RL.RelocResult()
        check(self._L.dvs_backend_relocalize_frame(self._h, relocalizer.handle, map_tracker.handle, M._raw(d_kps), M._raw(d_desc), int(n_kp), C.byref(r)))
        return r.as_dict()

    # ---- covisibility (include/dvslam_hip.h "Covisibility")
    def covisibility(self, min_weight=15, weights=True):
        """dvs_backend_covisibility: the whole graph -> dict(weights (n, n) int32 or None, nb_offsets (n + 1) int64, nb_index, nb_weight): the
        neighbour lists of every keyframe at min_weight as CSR, each ordered by (weight descending, index ascending)"""
        nk, nn = C.c_int32(), C.c_int64()
        check(self._L.dvs_backend_covisibility(self._h, int(min_weight), 0, 0, None, None, None, None, C.byref(nk), C.byref(nn)))
        n, m = nk.value, nn.value
        W = np.zeros((n, n), np.int32) if weights else None
        offs = np.zeros(n + 1, np.int64); idx = np.zeros(max(m, 1), np.int32); wt = np.zeros(max(m, 1), np.int32)
        check(self._L.dvs_backend_covisibility(self._h, int(min_weight), n, m, ptr(W) if weights else None, ptr(offs), ptr(idx), ptr(wt), C.byref(nk), C.byref(nn)))
        return dict(weights=W, nb_offsets=offs, nb_index=idx[:m], nb_weight=wt[:m])

    def local_window(self, ref_frame_id, **params):
        """dvs_backend_get_local_window of keyframe ref_frame_id (params: the fields of dvs_covis_params): window()'s dict plus kf_fixed,
        kf_weight and n_left_out"""
        p = covis_params(**params)
        nk, no, nl, left = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        none = [None] * 5
        check(self._L.dvs_backend_get_local_window(self._h, int(ref_frame_id), C.byref(p), 0, 0, 0, *none, C.byref(nk), *none, C.byref(no), None, None, None,
                                                   C.byref(nl), C.byref(left)))
        ck, co, cl = max(nk.value, 1), max(no.value, 1), max(nl.value, 1)
        kid = np.zeros(ck, np.uint64); R = np.zeros((ck, 3, 3)); t = np.zeros((ck, 3)); fixed = np.zeros(ck, np.uint8); kw = np.zeros(ck, np.int32)
        px = np.zeros((co, 2), np.float32); olm = np.zeros(co, np.uint64); ocl = np.zeros(co, np.int32); ofr = np.zeros(co, np.uint64); oix = np.zeros(co, np.int32)
        lid = np.zeros(cl, np.uint64); lcl = np.zeros(cl, np.int32); xyz = np.zeros((cl, 3), np.float32)
        check(self._L.dvs_backend_get_local_window(self._h, int(ref_frame_id), C.byref(p), ck, co, cl, ptr(kid), ptr(R), ptr(t), ptr(fixed), ptr(kw), C.byref(nk),
                                                   ptr(px), ptr(olm), ptr(ocl), ptr(ofr), ptr(oix), C.byref(no), ptr(lid), ptr(lcl), ptr(xyz), C.byref(nl), C.byref(left)))
        nk, no, nl = nk.value, no.value, nl.value
        return dict(kf_frame_id=kid[:nk], kf_R=R[:nk], kf_t=t[:nk], kf_fixed=fixed[:nk], kf_weight=kw[:nk], obs_px=px[:no], obs_landmark_id=olm[:no],
                    obs_class=ocl[:no], obs_frame_id=ofr[:no], obs_lm_index=oix[:no], lm_id=lid[:nl], lm_class=lcl[:nl], lm_xyz=xyz[:nl], n_left_out=left.value)

    def local_bundle_adjust(self, ref_frame_id, ba=None, **params):
        """dvs_backend_local_ba: the local window of keyframe ref_frame_id refined by BAProblem.solve_device on `ba` (a dvslam_amd.BAProblem of
        the same device; None: a handle this object creates once and keeps).  The map changes only if the solve converged
        (summary.termination == 0).  -> dict(summary=dvs_ba_summary, n_cameras, n_fixed, n_landmarks, n_observations, n_left_out, n_dropped)"""
        from .ba import BAProblem
        if ba is None:
            if self._gba is None:
                self._gba = BAProblem.empty(self.device)
            ba = self._gba
        p = covis_params(**params)
        r = LocalBaResult()
        check(self._L.dvs_backend_local_ba(self._h, ba._h, int(ref_frame_id), C.byref(p), C.byref(r)))
        out = {k: int(getattr(r, k)) for k, _ in LocalBaResult._fields_ if k != "summary"}
        out["summary"] = r.summary
        return out

    def track_frame_local(self, map_tracker, ref_frame_id, d_kps, d_desc, n_kp, R, t, **params):
        """dvs_backend_track_frame_local: track_frame against the local map of keyframe ref_frame_id only; map_tracker.matches() then reports
        rows of that local map, and the ids identify them"""
        from . import map_track as M
        M._bind(self._L)
        p = covis_params(**params)
        R = np.ascontiguousarray(R, np.float64).reshape(9); t = np.ascontiguousarray(t, np.float64).reshape(3)
        r = M.MapTrackResult()
        check(self._L.dvs_backend_track_frame_local(self._h, map_tracker.handle, int(ref_frame_id), C.byref(p), M._raw(d_kps), M._raw(d_desc), int(n_kp), ptr(R), ptr(t),
                                                    C.byref(r)))
        return r.as_dict()

    # ---- keyframe culling (include/dvslam_hip.h "Keyframe culling")
    def cull_keyframes(self, ref_frame_id=None, protected=(), apply=True, **params):
        """dvs_backend_cull_keyframes: redundant keyframes leave the map (apply=False: a dry run that only reports).  ref_frame_id None: every
        keyframe is in scope; else only the covisibility neighbours of that keyframe at min_weight.  protected: frame ids that are never culled.
        params: the fields of dvs_cull_params but `local`.  -> dict of the fields of dvs_cull_result plus culled_frame_id (uint64, ascending
        index) and, per keyframe in table order before the call, kf_observed, kf_redundant (int32) and kf_state (uint8: 0 out of scope,
        1 protected, 2 kept, 3 culled)"""
        if "local" in params:
            raise TypeError("local follows from ref_frame_id")
        p = cull_params(local=0 if ref_frame_id is None else 1, **params)
        prot = np.array([int(f) for f in protected], np.uint64)
        n = max(self.counts()["n_keyframes"], 1)
        fid = np.zeros(n, np.uint64); seen = np.zeros(n, np.int32); red = np.zeros(n, np.int32); state = np.zeros(n, np.uint8)
        r = CullResult(); nk = C.c_int32()
        check(self._L.dvs_backend_cull_keyframes(self._h, 0 if ref_frame_id is None else int(ref_frame_id), C.byref(p), ptr(prot) if len(prot) else None, len(prot),
                                                 1 if apply else 0, C.byref(r), n, ptr(fid), ptr(seen), ptr(red), ptr(state), C.byref(nk)))
        out = {k: int(getattr(r, k)) for k, _ in CullResult._fields_ if k != "reserved"}
        out.update(culled_frame_id=fid[:r.n_culled], kf_observed=seen[:nk.value], kf_redundant=red[:nk.value], kf_state=state[:nk.value])
        return out

    # ---- landmark refresh (include/dvslam_hip.h "Landmark refresh")
    def refresh_landmarks(self, scope_frame_id=None, **params):
        """dvs_backend_refresh_landmarks: every landmark in scope (scope_frame_id None: the whole table; else the landmarks that keyframe
        observes) gets the descriptor of the view with the smallest median distance to its other views.  params: update_descriptors,
        min_views.  -> dict of the fields of dvs_lm_refresh_result"""
        p = lm_refresh_params(scope_frame_id, **params)
        r = LmRefreshResult()
        check(self._L.dvs_backend_refresh_landmarks(self._h, C.byref(p), C.byref(r)))
        return {k: int(getattr(r, k)) for k, _ in LmRefreshResult._fields_}

    def landmark_geometry(self):
        """dvs_backend_get_landmark_geometry, a dry run over the whole table -> dict(normal (n, 3) float64, range (n, 2) float64 (dmin, dmax),
        n_counted int32, best_obs_id uint64, best_median int32), rows as landmarks()"""
        nn = C.c_int32()
        check(self._L.dvs_backend_get_landmark_geometry(self._h, 0, None, None, None, None, None, C.byref(nn)))
        n = nn.value
        c = max(n, 1)
        normal = np.zeros((c, 3)); rng = np.zeros((c, 2)); cnt = np.zeros(c, np.int32); oid = np.zeros(c, np.uint64); med = np.zeros(c, np.int32)
        check(self._L.dvs_backend_get_landmark_geometry(self._h, c, ptr(normal), ptr(rng), ptr(cnt), ptr(oid), ptr(med), C.byref(nn)))
        return dict(normal=normal[:n], range=rng[:n], n_counted=cnt[:n], best_obs_id=oid[:n], best_median=med[:n])

    def track_frame_gated(self, map_tracker, d_kps, d_desc, n_kp, R, t, **gates):
        """dvs_backend_track_frame_gated: track_frame with the distance and viewing-angle gates (gates: cos_min, range_factor); the geometry
        is computed for the table as it stands; map_tracker.gate_counts() then tells what each gate removed"""
        from . import map_track as M
        M._bind(self._L)
        g = maptrack_gates(**gates)
        R = np.ascontiguousarray(R, np.float64).reshape(9); t = np.ascontiguousarray(t, np.float64).reshape(3)
        r = M.MapTrackResult()
        check(self._L.dvs_backend_track_frame_gated(self._h, map_tracker.handle, C.byref(g), M._raw(d_kps), M._raw(d_desc), int(n_kp), ptr(R), ptr(t), C.byref(r)))
        return r.as_dict()

    # ---- landmark culling (include/dvslam_hip.h "Landmark culling")
    def set_tracking_stats(self, on=True):
        """dvs_backend_set_tracking_stats: while on, track_frame, track_frame_gated and track_frame_local record per landmark whether it was
        predicted visible and whether it was found"""
        check(self._L.dvs_backend_set_tracking_stats(self._h, 1 if on else 0))

    def landmark_stats(self):
        """dvs_backend_get_landmark_stats -> dict(id uint64, visible, found, n_views, age_kf int32, rows as landmarks(); n_frames_recorded int)"""
        nn, nf = C.c_int32(), C.c_int64()
        check(self._L.dvs_backend_get_landmark_stats(self._h, 0, None, None, None, None, None, C.byref(nn), C.byref(nf)))
        n = nn.value
        c = max(n, 1)
        lid = np.zeros(c, np.uint64); vis = np.zeros(c, np.int32); fnd = np.zeros(c, np.int32); nv = np.zeros(c, np.int32); age = np.zeros(c, np.int32)
        check(self._L.dvs_backend_get_landmark_stats(self._h, c, ptr(lid), ptr(vis), ptr(fnd), ptr(nv), ptr(age), C.byref(nn), C.byref(nf)))
        return dict(id=lid[:n], visible=vis[:n], found=fnd[:n], n_views=nv[:n], age_kf=age[:n], n_frames_recorded=int(nf.value))

    def set_landmark_stats(self, ids, visible, found):
        """dvs_backend_set_landmark_stats: ids strictly ascending; ids the map does not hold are skipped"""
        lid = np.ascontiguousarray(ids, np.uint64); vis = np.ascontiguousarray(visible, np.int32); fnd = np.ascontiguousarray(found, np.int32)
        if not len(lid) == len(vis) == len(fnd):
            raise ValueError("ids, visible and found must have one entry per row")
        check(self._L.dvs_backend_set_landmark_stats(self._h, len(lid), ptr(lid), ptr(vis), ptr(fnd)))

    def clear_landmark_stats(self):
        check(self._L.dvs_backend_clear_landmark_stats(self._h))

    def cull_landmarks(self, apply=True, cap=None, **params):
        """dvs_backend_cull_landmarks: the landmarks found in too few of the frames that predicted them, and the weak ones, leave the map
        (apply=False: a dry run that only reports).  params: the fields of dvs_lm_cull_params.  cap None: as many entries as the map has
        landmarks.  -> dict of the fields of dvs_lm_cull_result plus culled_id (uint64, ascending) and culled_reason (int32: 1 found
        ratio, 2 weak)"""
        p = lm_cull_params(**params)
        n = max(self.counts()["n_landmarks"], 1) if cap is None else int(cap)
        cid = np.zeros(max(n, 1), np.uint64); why = np.zeros(max(n, 1), np.int32)
        r = LmCullResult(); nc = C.c_int32()
        check(self._L.dvs_backend_cull_landmarks(self._h, C.byref(p), 1 if apply else 0, C.byref(r), n, ptr(cid), ptr(why), C.byref(nc)))
        out = {k: int(getattr(r, k)) for k, _ in LmCullResult._fields_ if k != "reserved"}
        out.update(culled_id=cid[:nc.value], culled_reason=why[:nc.value])
        return out

    def reset(self):
        check(self._L.dvs_backend_reset(self._h))

    def close(self):
        if getattr(self, "_h", None):
            self._L.dvs_backend_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


__all__ = ["MappingBackend", "BackendParams", "BackendResult", "Detection", "FuseParams", "FuseResult", "CloseLoopResult", "GlobalBaResult", "CovisParams", "LocalBaResult", "covis_params", "CullParams", "CullResult", "cull_params", "LmRefreshParams", "LmRefreshResult", "MapTrackGates", "LmCullParams", "LmCullResult", "lm_cull_params", "lm_refresh_params", "maptrack_gates", "default_params", "fuse_params", "DvsError"]
