"""ctypes mirror of the relocalisation (include/dvslam_hip.h, dvs_reloc_*): a frame's pose in the map without a prior — every landmark
searches all keypoints, the keypoints keep one landmark each, P3P RANSAC finds a pose on the kept pairs and a MapTracker confirms it."""
import ctypes as C
import numpy as np
from ._lib import lib, test_lib, check, ptr, KP_DTYPE
from .map_track import MapTrackResult, _raw

OK, FEW_PAIRS, NO_POSE, NOT_CONFIRMED = 0, 1, 2, 3

# dvs_reloc_lm_record (include/dvslam_hip_test_reloc.h), 20 bytes
LM_RECORD = np.dtype([("best_k", "<i4"), ("d_best", "<i4"), ("d_second", "<i4"), ("proposed", "<i4"), ("kept", "<i4")])


class RelocParams(C.Structure):
    _fields_ = [("K4", C.c_double * 4), ("max_hamming", C.c_int32), ("ratio_pct", C.c_int32), ("min_pairs", C.c_int32), ("pnp_iterations", C.c_int32),
                ("pnp_reproj_err", C.c_double), ("pnp_confidence", C.c_double), ("min_pnp_inliers", C.c_int32), ("min_confirmed", C.c_int32),
                ("seed", C.c_uint64)]


class RelocResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_proposed", C.c_int32), ("n_pairs", C.c_int32), ("pnp_inliers", C.c_int32), ("pnp_success", C.c_int32),
                ("reserved", C.c_int32), ("pnp_R", C.c_double * 9), ("pnp_t", C.c_double * 3), ("track", MapTrackResult), ("R", C.c_double * 9),
                ("t", C.c_double * 3)]

    INT_FIELDS = ("status", "n_proposed", "n_pairs", "pnp_inliers", "pnp_success")

    def as_dict(self):
        d = {k: int(getattr(self, k)) for k in self.INT_FIELDS}
        d.update(pnp_R=np.array(self.pnp_R[:]).reshape(3, 3), pnp_t=np.array(self.pnp_t[:]), track=self.track.as_dict(),
                 R=np.array(self.R[:]).reshape(3, 3), t=np.array(self.t[:]), raw=bytes(self))
        return d


def _bind(L):
    vp, i32 = C.c_void_p, C.c_int32
    pr = C.POINTER(RelocResult)
    L.dvs_reloc_default_params.argtypes = [C.POINTER(RelocParams)]; L.dvs_reloc_default_params.restype = None
    L.dvs_reloc_create.argtypes = [C.POINTER(RelocParams), i32, C.POINTER(vp)]
    L.dvs_reloc_destroy.argtypes = [vp]; L.dvs_reloc_destroy.restype = None
    L.dvs_reloc_set_stream.argtypes = [vp, vp]
    L.dvs_reloc_locate_device.argtypes = [vp, vp, vp, vp, vp, i32, vp, vp, i32, pr]
    L.dvs_reloc_locate.argtypes = [vp, vp, vp, vp, vp, i32, vp, vp, i32, pr]
    L.dvs_reloc_get_pairs.argtypes = [vp, i32, vp, vp, vp, vp, C.POINTER(i32)]
    L.dvs_reloc_set_timing.argtypes = [vp, i32]
    L.dvs_reloc_get_stage_ms.argtypes = [vp, vp]
    L.dvs_backend_relocalize_frame.argtypes = [vp, vp, vp, vp, vp, i32, pr]
    L.dvs_tracker_relocalize.argtypes = [vp, vp, vp, vp, i32, pr]
    if hasattr(L, "dvs_test_reloc_landmarks"):
        L.dvs_test_reloc_landmarks.argtypes = [vp, i32, vp, C.POINTER(i32)]
        L.dvs_test_reloc_pnp_record.argtypes = [vp, C.POINTER(i32), C.POINTER(i32), vp, vp]
    return L


def default_params(fx=0.0, fy=0.0, cx=0.0, cy=0.0, **kw):
    """dvs_reloc_default_params with the intrinsics and any field overrides"""
    p = RelocParams()
    _bind(lib()).dvs_reloc_default_params(C.byref(p))
    p.K4[0], p.K4[1], p.K4[2], p.K4[3] = fx, fy, cx, cy
    for k, v in kw.items():
        if k not in dict(RelocParams._fields_) or k == "K4":
            raise AttributeError(k)
        setattr(p, k, v)
    return p


class Relocalizer:
    """rl = Relocalizer(default_params(f, f, cx, cy)); r = rl.locate(map_tracker, xyz, ldesc, ids, kps, kdesc) -> result dict with the
    camera-to-world pose in r["R"], r["t"] when r["status"] == OK.  map_tracker: the MapTracker that confirms (its image size and
    intrinsics are the frame's).  hooks=True makes every call through lib/libdvslam_hip_test.so, which also has landmark_records()."""

    def __init__(self, params, device=0, hooks=False):
        self._L = _bind(test_lib() if hooks else lib())
        self._h = None
        self.params = params
        self.device = device
        h = C.c_void_p()
        check(self._L.dvs_reloc_create(C.byref(params), device, C.byref(h)))
        self._h = h

    @property
    def handle(self):
        return self._h

    def set_stream(self, stream):
        check(self._L.dvs_reloc_set_stream(self._h, stream))

    def locate_device(self, map_tracker, d_xyz, d_ldesc, d_ids, n_lm, d_kps, d_kdesc, n_kp):
        """on raw pointers (ints or DeviceBuffer; d_ids may be None)"""
        r = RelocResult()
        check(self._L.dvs_reloc_locate_device(self._h, map_tracker.handle, _raw(d_xyz), _raw(d_ldesc), _raw(d_ids), n_lm, _raw(d_kps), _raw(d_kdesc), n_kp,
                                              C.byref(r)))
        return r.as_dict()

    def locate(self, map_tracker, xyz, ldesc, ids, kps, kdesc):
        """host form: xyz float32 (n_lm, 3), ldesc uint8 (n_lm, 32), ids int64 ascending or None, kps KP_DTYPE, kdesc uint8 (n_kp, 32)"""
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3); ldesc = np.ascontiguousarray(ldesc, np.uint8).reshape(-1, 32)
        kps = np.ascontiguousarray(kps, KP_DTYPE); kdesc = np.ascontiguousarray(kdesc, np.uint8).reshape(-1, 32)
        ids = None if ids is None else np.ascontiguousarray(ids, np.int64)
        if len(ldesc) != len(xyz) or len(kdesc) != len(kps) or (ids is not None and len(ids) != len(xyz)):
            raise ValueError("row counts differ")
        r = RelocResult()
        check(self._L.dvs_reloc_locate(self._h, map_tracker.handle, ptr(xyz), ptr(ldesc), ptr(ids), len(xyz), ptr(kps), ptr(kdesc), len(kps), C.byref(r)))
        return r.as_dict()

    def pairs(self):
        """the last call's stage-3 list -> (lm_row int32, kp_index int32, dist int32, pnp_inlier uint8)"""
        n = C.c_int32()
        check(self._L.dvs_reloc_get_pairs(self._h, 0, None, None, None, None, C.byref(n)))
        m = n.value
        row = np.empty(m, np.int32); kp = np.empty(m, np.int32); dist = np.empty(m, np.int32); inl = np.empty(m, np.uint8)
        check(self._L.dvs_reloc_get_pairs(self._h, m, ptr(row), ptr(kp), ptr(dist), ptr(inl), C.byref(n)))
        return row, kp, dist, inl

    def set_timing(self, on=True):
        check(self._L.dvs_reloc_set_timing(self._h, 1 if on else 0))

    def stage_ms(self):
        """(timing on) device-event times of the last call -> {stage1, stage23, stage4} in ms"""
        ms = np.zeros(3)
        check(self._L.dvs_reloc_get_stage_ms(self._h, ptr(ms)))
        return dict(stage1=float(ms[0]), stage23=float(ms[1]), stage4=float(ms[2]))

    def landmark_records(self):
        """(hooks) the per-landmark records of the last call"""
        n = C.c_int32()
        check(self._L.dvs_test_reloc_landmarks(self._h, 0, None, C.byref(n)))
        rec = np.zeros(n.value, LM_RECORD)
        check(self._L.dvs_test_reloc_landmarks(self._h, n.value, ptr(rec), C.byref(n)))
        return rec

    def pnp_record(self):
        """(hooks) stage 4's record of the last call -> (success, rvec, tvec, n_inliers)"""
        n, ok = C.c_int32(), C.c_int32()
        rvec = np.zeros(3); tvec = np.zeros(3)
        check(self._L.dvs_test_reloc_pnp_record(self._h, C.byref(n), C.byref(ok), ptr(rvec), ptr(tvec)))
        return bool(ok.value), rvec, tvec, n.value

    def close(self):
        if getattr(self, "_h", None):
            self._L.dvs_reloc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


__all__ = ["Relocalizer", "RelocParams", "RelocResult", "default_params", "LM_RECORD", "OK", "FEW_PAIRS", "NO_POSE", "NOT_CONFIRMED"]
