"""ctypes mirror of the motion segmentation (include/dvslam_hip.h, dvs_motion_*): two depth images, their relative pose and the intrinsics ->
the 8-bit keep mask the extractor's masked entry points read (255 = keep, 0 = moving)."""
import ctypes as C
import numpy as np
from ._lib import lib, test_lib, check, ptr, DeviceBuffer


class MotionParams(C.Structure):
    _fields_ = [("rows", C.c_int32), ("cols", C.c_int32), ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                ("min_depth_mm", C.c_int32), ("max_depth_mm", C.c_int32), ("tau0_m", C.c_double), ("tau2_per_m", C.c_double),
                ("min_area", C.c_int32), ("dilate_radius", C.c_int32)]


class MotionStats(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("n_valid", "n_seed", "n_components", "n_components_kept", "n_dynamic", "n_masked")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


def _bind(L):
    vp, i32, sz = C.c_void_p, C.c_int32, C.c_size_t
    L.dvs_motion_default_params.argtypes = [C.POINTER(MotionParams)]; L.dvs_motion_default_params.restype = None
    L.dvs_motion_create.argtypes = [C.POINTER(MotionParams), i32, C.POINTER(vp)]
    L.dvs_motion_destroy.argtypes = [vp]; L.dvs_motion_destroy.restype = None
    L.dvs_motion_set_stream.argtypes = [vp, vp]
    L.dvs_motion_segment_device.argtypes = [vp, vp, sz, vp, sz, vp, vp, vp, sz, C.POINTER(MotionStats)]
    L.dvs_motion_segment.argtypes = [vp, vp, sz, vp, sz, vp, vp, vp, sz, C.POINTER(MotionStats)]
    if hasattr(L, "dvs_test_motion_label"):
        L.dvs_test_motion_label.argtypes = [i32, vp, i32, i32, vp, vp]
        L.dvs_test_motion_stages.argtypes = [vp, vp, vp, vp]
    return L


def default_params(rows=0, cols=0, fx=0.0, fy=0.0, cx=0.0, cy=0.0, **kw):
    """dvs_motion_default_params with the image size, the intrinsics and any field overrides"""
    p = MotionParams()
    _bind(lib()).dvs_motion_default_params(C.byref(p))
    p.rows, p.cols, p.fx, p.fy, p.cx, p.cy = rows, cols, fx, fy, cx, cy
    for k, v in kw.items():
        if k not in dict(MotionParams._fields_):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def _depth(a, rows, cols):
    a = np.asarray(a)
    if a.dtype != np.uint16 or a.shape != (rows, cols):
        raise ValueError(f"depth must be uint16 {(rows, cols)}, got {a.dtype} {a.shape}")
    if a.strides[1] != 2 or a.strides[0] < cols * 2 or a.strides[0] % 2:
        a = np.ascontiguousarray(a)
    return a


class MotionSegmenter:
    """seg = MotionSegmenter(default_params(480, 640, f, f, cx, cy)); mask, stats = seg.segment(depth_ref, depth_cur, R, t) with
    X_ref = R X_cur + t.  hooks=True makes every call through lib/libdvslam_hip_test.so, which also has label() and stages()."""

    def __init__(self, params, device=0, hooks=False):
        self._L = _bind(test_lib() if hooks else lib())
        self._h = None
        self.params = params
        self.rows, self.cols = int(params.rows), int(params.cols)
        self.device = device
        h = C.c_void_p()
        check(self._L.dvs_motion_create(C.byref(params), device, C.byref(h)))
        self._h = h

    def set_stream(self, stream):
        check(self._L.dvs_motion_set_stream(self._h, stream))

    @staticmethod
    def _pose(R, t):
        return np.ascontiguousarray(R, np.float64).reshape(9), np.ascontiguousarray(t, np.float64).reshape(3)

    def segment(self, ref, cur, R, t, want_stats=True):
        """host form -> (mask uint8 (rows, cols), stats dict or None)"""
        ref, cur = _depth(ref, self.rows, self.cols), _depth(cur, self.rows, self.cols)
        R, t = self._pose(R, t)
        mask = np.empty((self.rows, self.cols), np.uint8)
        st = MotionStats()
        check(self._L.dvs_motion_segment(self._h, ptr(ref), ref.strides[0], ptr(cur), cur.strides[0], ptr(R), ptr(t), ptr(mask), self.cols,
                                         C.byref(st) if want_stats else None))
        return mask, (st.as_dict() if want_stats else None)

    def segment_device(self, d_ref, ref_step, d_cur, cur_step, R, t, d_mask, mask_step, want_stats=False):
        """device form on raw pointers (ints or DeviceBuffer): asynchronous unless want_stats -> stats dict or None"""
        R, t = self._pose(R, t)
        raw = [b.ptr if isinstance(b, DeviceBuffer) else b for b in (d_ref, d_cur, d_mask)]
        st = MotionStats()
        check(self._L.dvs_motion_segment_device(self._h, raw[0], ref_step, raw[1], cur_step, ptr(R), ptr(t), raw[2], mask_step,
                                                C.byref(st) if want_stats else None))
        return st.as_dict() if want_stats else None

    def stages(self):
        """(hooks) the last call's seed image, labels and dynamic image"""
        n = self.rows * self.cols
        seed = np.empty(n, np.uint8); lab = np.empty(n, np.int32); dyn = np.empty(n, np.uint8)
        check(self._L.dvs_test_motion_stages(self._h, ptr(seed), ptr(lab), ptr(dyn)))
        return seed.reshape(self.rows, self.cols), lab.reshape(self.rows, self.cols), dyn.reshape(self.rows, self.cols)

    def close(self):
        if getattr(self, "_h", None):
            self._L.dvs_motion_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def label_image(img, device=0):
    """(hooks) dvs_test_motion_label: the labelling launches on a binary image -> (labels int32, areas int32), both img's shape"""
    L = _bind(test_lib())
    img = np.ascontiguousarray(img, np.uint8)
    rows, cols = img.shape
    lab = np.empty(img.shape, np.int32); area = np.empty(img.shape, np.int32)
    check(L.dvs_test_motion_label(device, ptr(img), rows, cols, ptr(lab), ptr(area)))
    return lab, area


__all__ = ["MotionSegmenter", "MotionParams", "MotionStats", "default_params", "label_image"]
