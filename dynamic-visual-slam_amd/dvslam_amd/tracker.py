"""ctypes mirror of the tracking front end (include/dvslam_hip.h, dvs_tracker_*): Frontend::syncCallback (frontend.cpp:1068-1324) as one
handle and one call per RGB-D frame, device-resident between the image upload and the result record."""
import ctypes as C
import numpy as np
from ._lib import lib, check, ptr, KP_DTYPE, OrbParams, DvsError
from .motion import MotionParams, MotionStats

KF_FIRST_FRAME, KF_NO_REFERENCE, KF_FEW_MATCHES, KF_MAX_FRAMES = 1, 2, 4, 8


class TrackerParams(C.Structure):
    _fields_ = [("rows", C.c_int32), ("cols", C.c_int32), ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                ("orb", OrbParams), ("min_depth", C.c_float), ("max_depth", C.c_float), ("max_hamming", C.c_int32),
                ("fm_threshold", C.c_double), ("fm_confidence", C.c_double), ("fm_max_iters", C.c_int32), ("cull_max_new", C.c_int32),
                ("cull_min_response", C.c_float), ("pnp_iterations", C.c_int32), ("pnp_reproj_err", C.c_double), ("pnp_confidence", C.c_double),
                ("kf_min_matches", C.c_int32), ("kf_max_frames", C.c_int32), ("max_translation", C.c_double), ("max_rotation", C.c_double),
                ("fm_mode", C.c_int32), ("pnp_mode", C.c_int32), ("seed_base", C.c_uint64), ("gray_variant", C.c_int32), ("reserved", C.c_int32)]


class TrackResult(C.Structure):
    _fields_ = [("frame_index", C.c_int64), ("keyframe_id", C.c_int64), ("n_extracted", C.c_int32), ("n_filtered", C.c_int32),
                ("n_matches", C.c_int32), ("n_geometric", C.c_int32), ("n_pnp_points", C.c_int32), ("n_pnp_inliers", C.c_int32),
                ("n_backend", C.c_int32), ("n_kf_matches", C.c_int32), ("n_kf_geometric", C.c_int32), ("first_frame", C.c_int32),
                ("tracking_reset", C.c_int32), ("fm_skipped", C.c_int32), ("pnp_skipped", C.c_int32), ("pnp_failed", C.c_int32),
                ("motion_outlier", C.c_int32), ("pose_updated", C.c_int32), ("is_keyframe", C.c_int32), ("kf_criterion", C.c_int32),
                ("cdr_landmarks", C.c_int32), ("reserved", C.c_int32), ("cdr_bytes", C.c_uint64), ("rvec", C.c_double * 3),
                ("tvec", C.c_double * 3), ("R", C.c_double * 9), ("t", C.c_double * 3)]

    INT_FIELDS = ("frame_index", "keyframe_id", "n_extracted", "n_filtered", "n_matches", "n_geometric", "n_pnp_points", "n_pnp_inliers", "n_backend",
                  "n_kf_matches", "n_kf_geometric", "first_frame", "tracking_reset", "fm_skipped", "pnp_skipped", "pnp_failed", "motion_outlier",
                  "pose_updated", "is_keyframe", "kf_criterion", "cdr_landmarks", "cdr_bytes")

    def as_dict(self):
        d = {k: int(getattr(self, k)) for k in self.INT_FIELDS}
        d.update(rvec=np.array(self.rvec[:]), tvec=np.array(self.tvec[:]), R=np.array(self.R[:]).reshape(3, 3), t=np.array(self.t[:]))
        return d


def _bind(L):
    vp, i32, sz = C.c_void_p, C.c_int32, C.c_size_t
    L.dvs_tracker_default_params.argtypes = [C.POINTER(TrackerParams)]; L.dvs_tracker_default_params.restype = None
    L.dvs_tracker_create.argtypes = [C.POINTER(TrackerParams), i32, C.POINTER(vp)]
    L.dvs_tracker_destroy.argtypes = [vp]; L.dvs_tracker_destroy.restype = None
    L.dvs_tracker_reset.argtypes = [vp]
    L.dvs_tracker_set_stream.argtypes = [vp, vp]
    L.dvs_tracker_synchronize.argtypes = [vp]
    L.dvs_tracker_track.argtypes = [vp, vp, i32, sz, vp, sz, i32, C.c_uint32, C.POINTER(TrackResult), vp, sz]
    L.dvs_tracker_get_backend_features.argtypes = [vp, vp, vp, vp, i32, C.POINTER(i32)]
    L.dvs_tracker_set_motion_mask.argtypes = [vp, C.POINTER(MotionParams), i32]
    L.dvs_tracker_get_motion_mask.argtypes = [vp, vp, sz, vp, vp, C.POINTER(C.c_int64), C.POINTER(MotionStats)]
    L.dvs_keyframe_cdr_capacity.argtypes = [C.c_char_p, i32]; L.dvs_keyframe_cdr_capacity.restype = sz
    return L


def default_params(rows=0, cols=0, fx=0.0, fy=0.0, cx=0.0, cy=0.0, **kw):
    """dvs_tracker_default_params (the reference's constants) with the frame size, the intrinsics and any field overrides"""
    p = TrackerParams()
    _bind(lib()).dvs_tracker_default_params(C.byref(p))
    p.rows, p.cols, p.fx, p.fy, p.cx, p.cy = rows, cols, fx, fy, cx, cy
    for k, v in kw.items():
        if k == "nfeatures":
            p.orb.nfeatures = v
        elif not hasattr(p, k):
            raise AttributeError(k)
        else:
            setattr(p, k, v)
    return p


def validate_frame(image, depth, rows, cols):
    """shape / dtype rules of Tracker.track, checked before anything reaches the library -> (image, depth, channels)"""
    image = np.asarray(image); depth = np.asarray(depth)
    if image.dtype != np.uint8 or image.ndim not in (2, 3) or (image.ndim == 3 and image.shape[2] != 3):
        raise ValueError(f"image must be uint8 (rows, cols) or (rows, cols, 3), got {image.dtype} {image.shape}")
    if image.shape[:2] != (rows, cols):
        raise ValueError(f"image is {image.shape[:2]}, the tracker was made for {(rows, cols)}")
    if depth.dtype != np.uint16 or depth.shape != (rows, cols):
        raise ValueError(f"depth must be uint16 {(rows, cols)}, got {depth.dtype} {depth.shape}")
    ch = 1 if image.ndim == 2 else 3
    if image.strides[-1] != 1 or (ch == 3 and image.strides[1] != 3) or image.strides[0] < cols * ch:
        image = np.ascontiguousarray(image)
    if depth.strides[1] != 2 or depth.strides[0] < cols * 2:
        depth = np.ascontiguousarray(depth)
    return image, depth, ch


class Tracker:
    """tr = Tracker(default_params(480, 640, f, f, cx, cy)); r, payload = tr.track(image, depth, (sec, nanosec))"""

    def __init__(self, params, device=0):
        self._L = _bind(lib())
        self._h = None
        self.params = params
        self.rows, self.cols = int(params.rows), int(params.cols)
        h = C.c_void_p()
        check(self._L.dvs_tracker_create(C.byref(params), device, C.byref(h)))
        self._h = h
        cap = params.orb.nfeatures + 3 * params.orb.nlevels
        self.capacity = cap
        self._cdr = np.zeros(self._L.dvs_keyframe_cdr_capacity(b"camera_link", cap), np.uint8)

    def track(self, image, depth, stamp=(0, 0), want_payload=True):
        """one frame: image uint8 (rows, cols) or BGR (rows, cols, 3), depth uint16 (rows, cols) in millimetres
        -> (result dict, Keyframe.msg CDR bytes or None)"""
        image, depth, ch = validate_frame(image, depth, self.rows, self.cols)
        if self._h is None:
            raise RuntimeError("tracker is closed")
        r = TrackResult()
        check(self._L.dvs_tracker_track(self._h, ptr(image), ch, image.strides[0], ptr(depth), depth.strides[0], int(stamp[0]), int(stamp[1]), C.byref(r),
                                        ptr(self._cdr) if want_payload else None, self._cdr.nbytes))
        d = r.as_dict()
        payload = self._cdr[:d["cdr_bytes"]].tobytes() if (want_payload and d["is_keyframe"]) else None
        return d, payload

    def backend_features(self):
        """the last frame's culled set, in order -> (keypoints, descriptors, indices into the depth-filtered set)"""
        k = np.zeros(self.capacity, KP_DTYPE); d = np.zeros((self.capacity, 32), np.uint8); s = np.zeros(self.capacity, np.int32); n = C.c_int32()
        check(self._L.dvs_tracker_get_backend_features(self._h, ptr(k), ptr(d), ptr(s), self.capacity, C.byref(n)))
        return k[:n.value].copy(), d[:n.value].copy(), s[:n.value].copy()

    def track_map(self, backend, map_tracker, apply=False):
        """dvs_tracker_track_map: the last frame's depth-filtered features against the backend's landmark table, prior R_, t_ -> map_track
        result dict; apply=True and status 0: the refined pose replaces R_, t_"""
        from . import map_track as M
        M._bind(self._L)
        r = M.MapTrackResult()
        check(self._L.dvs_tracker_track_map(self._h, backend._h, map_tracker.handle, 1 if apply else 0, C.byref(r)))
        return r.as_dict()

    def relocalize(self, backend, relocalizer, map_tracker, apply=False):
        """dvs_tracker_relocalize: the last frame's depth-filtered features against the backend's landmark table with no prior -> reloc result
        dict; apply=True and status 0: the found pose replaces R_, t_"""
        from . import reloc as RL
        RL._bind(self._L)
        r = RL.RelocResult()
        check(self._L.dvs_tracker_relocalize(self._h, backend._h, relocalizer.handle, map_tracker.handle, 1 if apply else 0, C.byref(r)))
        return r.as_dict()

    def filtered_features(self):
        """the last frame's depth-filtered set -> (keypoints, descriptors)"""
        from . import map_track as M
        M._bind(self._L)
        k = np.zeros(self.capacity, KP_DTYPE); d = np.zeros((self.capacity, 32), np.uint8); n = C.c_int32()
        check(self._L.dvs_tracker_get_filtered_features(self._h, ptr(k), ptr(d), self.capacity, C.byref(n)))
        return k[:n.value].copy(), d[:n.value].copy()

    def set_motion_mask(self, params, lag=4):
        """dvs_tracker_set_motion_mask: params a motion.MotionParams (its size and intrinsics are replaced by the tracker's) or None to
        switch the motion mask off; lag in 1..16"""
        check(self._L.dvs_tracker_set_motion_mask(self._h, C.byref(params) if params is not None else None, int(lag)))

    def motion_mask(self):
        """what the last frame's extraction used -> (mask uint8 (rows, cols), R (3, 3), t (3,), reference frame index or -1, stats dict)"""
        mask = np.empty((self.rows, self.cols), np.uint8); R = np.empty(9); t = np.empty(3); ref = C.c_int64(); st = MotionStats()
        check(self._L.dvs_tracker_get_motion_mask(self._h, ptr(mask), self.cols, ptr(R), ptr(t), C.byref(ref), C.byref(st)))
        return mask, R.reshape(3, 3), t, int(ref.value), st.as_dict()

    def reset(self):
        check(self._L.dvs_tracker_reset(self._h))

    def synchronize(self):
        check(self._L.dvs_tracker_synchronize(self._h))

    def close(self):
        if getattr(self, "_h", None):
            self._L.dvs_tracker_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


__all__ = ["Tracker", "validate_frame", "TrackerParams", "TrackResult", "default_params", "DvsError", "KF_FIRST_FRAME", "KF_NO_REFERENCE", "KF_FEW_MATCHES", "KF_MAX_FRAMES"]
