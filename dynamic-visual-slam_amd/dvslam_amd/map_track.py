"""ctypes mirror of the tracking against the map (include/dvslam_hip.h, dvs_maptrack_*): landmarks projected into a frame, a descriptor
search in a window around each projection, a one-to-one assignment and the refinement of the frame's pose on the kept 3D-2D pairs."""
import ctypes as C
import numpy as np
from ._lib import lib, test_lib, check, ptr, KP_DTYPE, DeviceBuffer

OK, FEW_MATCHES, FEW_INLIERS, DEGENERATE = 0, 1, 2, 3
MAX_LEVELS = 16

# dvs_maptrack_lm_record (include/dvslam_hip_test_maptrack.h), 40 bytes
LM_RECORD = np.dtype([("u", "<f8"), ("v", "<f8"), ("visible", "<i4"), ("best_k", "<i4"), ("d_best", "<i4"), ("d_second", "<i4"),
                      ("proposed", "<i4"), ("kept", "<i4")])


class MapTrackParams(C.Structure):
    _fields_ = [("rows", C.c_int32), ("cols", C.c_int32), ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                ("min_z", C.c_double), ("max_z", C.c_double), ("radius", C.c_double), ("cell", C.c_int32), ("max_hamming", C.c_int32),
                ("ratio_pct", C.c_int32), ("reserved0", C.c_int32), ("chi2_gate", C.c_double), ("min_matches", C.c_int32),
                ("min_inliers", C.c_int32), ("n_levels", C.c_int32), ("reserved1", C.c_int32), ("level_sigma2", C.c_double * MAX_LEVELS)]


class MapTrackResult(C.Structure):
    _fields_ = [("R", C.c_double * 9), ("t", C.c_double * 3), ("cost", C.c_double), ("status", C.c_int32), ("n_visible", C.c_int32),
                ("n_proposed", C.c_int32), ("n_matches", C.c_int32), ("n_inliers", C.c_int32), ("n_unbinned", C.c_int32)]

    INT_FIELDS = ("status", "n_visible", "n_proposed", "n_matches", "n_inliers", "n_unbinned")

    def as_dict(self):
        d = {k: int(getattr(self, k)) for k in self.INT_FIELDS}
        d.update(R=np.array(self.R[:]).reshape(3, 3), t=np.array(self.t[:]), cost=float(self.cost))
        return d


def _bind(L):
    vp, i32 = C.c_void_p, C.c_int32
    pr = C.POINTER(MapTrackResult)
    L.dvs_maptrack_default_params.argtypes = [C.POINTER(MapTrackParams)]; L.dvs_maptrack_default_params.restype = None
    L.dvs_maptrack_create.argtypes = [C.POINTER(MapTrackParams), i32, C.POINTER(vp)]
    L.dvs_maptrack_destroy.argtypes = [vp]; L.dvs_maptrack_destroy.restype = None
    L.dvs_maptrack_set_stream.argtypes = [vp, vp]
    L.dvs_maptrack_search_device.argtypes = [vp, vp, vp, vp, i32, vp, vp, i32, vp, vp, pr]
    L.dvs_maptrack_refine_device.argtypes = [vp, vp, vp, vp, i32, vp, vp, pr]
    L.dvs_maptrack_track_device.argtypes = [vp, vp, vp, vp, i32, vp, vp, i32, vp, vp, pr]
    L.dvs_maptrack_track.argtypes = [vp, vp, vp, vp, i32, vp, vp, i32, vp, vp, pr]
    L.dvs_maptrack_get_matches.argtypes = [vp, i32, vp, vp, vp, vp, C.POINTER(i32)]
    L.dvs_backend_track_frame.argtypes = [vp, vp, vp, vp, i32, vp, vp, pr]
    L.dvs_backend_track_frame_local.argtypes = [vp, vp, C.c_uint64, vp, vp, vp, i32, vp, vp, pr]
    L.dvs_tracker_track_map.argtypes = [vp, vp, vp, i32, pr]
    L.dvs_tracker_get_filtered_features.argtypes = [vp, vp, vp, i32, C.POINTER(i32)]
    L.dvs_mapgate_search_device.argtypes = [vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, i32, vp, vp, pr]
    L.dvs_mapgate_track_device.argtypes = [vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, i32, vp, vp, pr]
    L.dvs_mapgate_get_counts.argtypes = [vp, vp]
    L.dvs_tracker_track_map_gated.argtypes = [vp, vp, vp, vp, i32, pr]
    if hasattr(L, "dvs_test_maptrack_landmarks"):
        L.dvs_test_maptrack_landmarks.argtypes = [vp, i32, vp, C.POINTER(i32)]
        L.dvs_test_maptrack_cells.argtypes = [vp, i32, i32, vp, vp, C.POINTER(i32), C.POINTER(i32)]
        L.dvs_test_maptrack_refine_steps.argtypes = [vp, vp, vp, vp, i32, vp, vp, i32, i32, i32, pr]
    return L


def default_params(rows=0, cols=0, fx=0.0, fy=0.0, cx=0.0, cy=0.0, level_sigma2=None, **kw):
    """dvs_maptrack_default_params with the image size, the intrinsics and any field overrides; level_sigma2: a sequence that replaces the
    table (n_levels follows its length unless given)"""
    p = MapTrackParams()
    _bind(lib()).dvs_maptrack_default_params(C.byref(p))
    p.rows, p.cols, p.fx, p.fy, p.cx, p.cy = rows, cols, fx, fy, cx, cy
    if level_sigma2 is not None:
        if len(level_sigma2) > MAX_LEVELS:
            raise ValueError(f"at most {MAX_LEVELS} levels")
        for k in range(MAX_LEVELS):
            p.level_sigma2[k] = float(level_sigma2[k]) if k < len(level_sigma2) else 0.0
        p.n_levels = len(level_sigma2)
    for k, v in kw.items():
        if k not in dict(MapTrackParams._fields_):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def _raw(b):
    return b.ptr if isinstance(b, DeviceBuffer) else b


def _pose(R, t):
    return np.ascontiguousarray(R, np.float64).reshape(9), np.ascontiguousarray(t, np.float64).reshape(3)


class MapTracker:
    """mt = MapTracker(default_params(480, 640, f, f, cx, cy)); r = mt.track(xyz, ldesc, ids, kps, kdesc, R, t) -> result dict with the
    refined camera-to-world pose when r["status"] == OK.  hooks=True makes every call through lib/libdvslam_hip_test.so, which also has
    landmark_records(), cells() and refine_steps()."""

    def __init__(self, params, device=0, hooks=False):
        self._L = _bind(test_lib() if hooks else lib())
        self._h = None
        self.params = params
        self.device = device
        h = C.c_void_p()
        check(self._L.dvs_maptrack_create(C.byref(params), device, C.byref(h)))
        self._h = h

    @property
    def handle(self):
        return self._h

    def set_stream(self, stream):
        check(self._L.dvs_maptrack_set_stream(self._h, stream))

    def search_device(self, d_xyz, d_ldesc, d_ids, n_lm, d_kps, d_kdesc, n_kp, R, t, want_counts=True):
        """stages 1-3 on raw pointers (ints or DeviceBuffer; d_ids may be None): asynchronous unless want_counts -> result dict or None"""
        R, t = _pose(R, t)
        r = MapTrackResult()
        check(self._L.dvs_maptrack_search_device(self._h, _raw(d_xyz), _raw(d_ldesc), _raw(d_ids), n_lm, _raw(d_kps), _raw(d_kdesc), n_kp, ptr(R), ptr(t),
                                                 C.byref(r) if want_counts else None))
        return r.as_dict() if want_counts else None

    def refine_device(self, d_X, d_px, d_octave, n, R, t):
        """stage 4 on explicit correspondences (device: n x 3 doubles, n x 2 doubles, n int32)"""
        R, t = _pose(R, t)
        r = MapTrackResult()
        check(self._L.dvs_maptrack_refine_device(self._h, _raw(d_X), _raw(d_px), _raw(d_octave), n, ptr(R), ptr(t), C.byref(r)))
        return r.as_dict()

    def refine_steps(self, d_X, d_px, d_octave, n, R, t, first_round=0, n_rounds=4, n_iters=10):
        """(hooks) refine_device with a part of its schedule: rounds first_round .. first_round + n_rounds - 1 of n_iters steps each"""
        R, t = _pose(R, t)
        r = MapTrackResult()
        check(self._L.dvs_test_maptrack_refine_steps(self._h, _raw(d_X), _raw(d_px), _raw(d_octave), n, ptr(R), ptr(t), first_round, n_rounds, n_iters,
                                                     C.byref(r)))
        return r.as_dict()

    def track_device(self, d_xyz, d_ldesc, d_ids, n_lm, d_kps, d_kdesc, n_kp, R, t):
        R, t = _pose(R, t)
        r = MapTrackResult()
        check(self._L.dvs_maptrack_track_device(self._h, _raw(d_xyz), _raw(d_ldesc), _raw(d_ids), n_lm, _raw(d_kps), _raw(d_kdesc), n_kp, ptr(R), ptr(t),
                                                C.byref(r)))
        return r.as_dict()

    def _gated(self, fn, d_xyz, d_ldesc, d_ids, n_lm, d_normal, d_range, d_ncounted, d_kps, d_kdesc, n_kp, R, t, gates, want):
        from .backend import maptrack_gates
        g = maptrack_gates(**gates)
        R, t = _pose(R, t)
        r = MapTrackResult()
        check(fn(self._h, _raw(d_xyz), _raw(d_ldesc), _raw(d_ids), n_lm, _raw(d_normal), _raw(d_range), _raw(d_ncounted), C.byref(g), _raw(d_kps), _raw(d_kdesc),
                 n_kp, ptr(R), ptr(t), C.byref(r) if want else None))
        return r.as_dict() if want else None

    def search_gated(self, d_xyz, d_ldesc, d_ids, n_lm, d_normal, d_range, d_ncounted, d_kps, d_kdesc, n_kp, R, t, want_counts=True, **gates):
        """search_device with the gates of "Landmark refresh": d_normal n_lm x 3 and d_range n_lm x 2 doubles, d_ncounted n_lm int32 on the
        device; gates: cos_min, range_factor"""
        return self._gated(self._L.dvs_mapgate_search_device, d_xyz, d_ldesc, d_ids, n_lm, d_normal, d_range, d_ncounted, d_kps, d_kdesc, n_kp, R, t, gates,
                           want_counts)

    def track_gated(self, d_xyz, d_ldesc, d_ids, n_lm, d_normal, d_range, d_ncounted, d_kps, d_kdesc, n_kp, R, t, **gates):
        """track_device with the gates"""
        return self._gated(self._L.dvs_mapgate_track_device, d_xyz, d_ldesc, d_ids, n_lm, d_normal, d_range, d_ncounted, d_kps, d_kdesc, n_kp, R, t, gates, True)

    def gate_counts(self):
        """what the last call's gates removed -> int32 [near, far, back-facing, angle]"""
        out = np.zeros(4, np.int32)
        check(self._L.dvs_mapgate_get_counts(self._h, ptr(out)))
        return out

    def track(self, xyz, ldesc, ids, kps, kdesc, R, t):
        """host form: xyz float32 (n_lm, 3), ldesc uint8 (n_lm, 32), ids int64 ascending or None, kps KP_DTYPE, kdesc uint8 (n_kp, 32)"""
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3); ldesc = np.ascontiguousarray(ldesc, np.uint8).reshape(-1, 32)
        kps = np.ascontiguousarray(kps, KP_DTYPE); kdesc = np.ascontiguousarray(kdesc, np.uint8).reshape(-1, 32)
        ids = None if ids is None else np.ascontiguousarray(ids, np.int64)
        if len(ldesc) != len(xyz) or len(kdesc) != len(kps) or (ids is not None and len(ids) != len(xyz)):
            raise ValueError("row counts differ")
        R, t = _pose(R, t)
        r = MapTrackResult()
        check(self._L.dvs_maptrack_track(self._h, ptr(xyz), ptr(ldesc), ptr(ids), len(xyz), ptr(kps), ptr(kdesc), len(kps), ptr(R), ptr(t), C.byref(r)))
        return r.as_dict()

    def matches(self):
        """the last call's per-keypoint arrays -> (lm_row int32, lm_id int64, dist int32, inlier uint8)"""
        n = C.c_int32()
        check(self._L.dvs_maptrack_get_matches(self._h, 0, None, None, None, None, C.byref(n)))
        m = n.value
        row = np.empty(m, np.int32); ids = np.empty(m, np.int64); dist = np.empty(m, np.int32); inl = np.empty(m, np.uint8)
        check(self._L.dvs_maptrack_get_matches(self._h, m, ptr(row), ptr(ids), ptr(dist), ptr(inl), C.byref(n)))
        return row, ids, dist, inl

    def landmark_records(self):
        """(hooks) the per-landmark records of the last search / track call"""
        n = C.c_int32()
        check(self._L.dvs_test_maptrack_landmarks(self._h, 0, None, C.byref(n)))
        rec = np.zeros(n.value, LM_RECORD)
        check(self._L.dvs_test_maptrack_landmarks(self._h, n.value, ptr(rec), C.byref(n)))
        return rec

    def cells(self):
        """(hooks) the cell CSR of the last search / track call -> (cell_start int32 [ncell + 1], order int32 [n_binned])"""
        nc, nb = C.c_int32(), C.c_int32()
        check(self._L.dvs_test_maptrack_cells(self._h, 0, 0, None, None, C.byref(nc), C.byref(nb)))
        start = np.zeros(nc.value + 1, np.int32); order = np.zeros(nb.value, np.int32)
        check(self._L.dvs_test_maptrack_cells(self._h, nc.value, nb.value, ptr(start), ptr(order), C.byref(nc), C.byref(nb)))
        return start, order

    def close(self):
        if getattr(self, "_h", None):
            self._L.dvs_maptrack_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


__all__ = ["MapTracker", "MapTrackParams", "MapTrackResult", "default_params", "LM_RECORD", "OK", "FEW_MATCHES", "FEW_INLIERS", "DEGENERATE"]
