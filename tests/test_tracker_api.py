"""The tracking front end's ABI without a GPU: the dvs_tracker_* block is declared and exported by both libraries, the culling hook by
the test library only, argument errors come before any device work, the defaults are the reference's constants, and the Python mirror
refuses bad frames before it calls the library."""
import ctypes as C
import os
import re
import subprocess
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["dvs_tracker_default_params", "dvs_tracker_create", "dvs_tracker_destroy", "dvs_tracker_reset", "dvs_tracker_set_stream",
           "dvs_tracker_synchronize", "dvs_tracker_track", "dvs_tracker_get_backend_features"]


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return set(line.split()[-1] for line in out.splitlines() if line.strip())


def test_symbols_declared_and_exported(hiplib, hooks):
    from dvslam_amd import _lib
    header = open(os.path.join(ROOT, "include", "dvslam_hip.h")).read()
    test_header = open(os.path.join(ROOT, "include", "dvslam_hip_test.h")).read()
    product, test = _exports(_lib.SO_PATH), _exports(_lib.TEST_SO_PATH)
    for s in SYMBOLS:
        assert re.search(r"\b" + s + r"\(", header), s
        assert s in product and s in test, s
    # the hook is declared in a header of its own that dvslam_hip_test.h includes (so it is declared for whoever includes that)
    hook_header = open(os.path.join(ROOT, "include", "dvslam_hip_test_tracker.h")).read()
    assert '#include "dvslam_hip_test_tracker.h"' in test_header and "dvs_test_cull_order(" in hook_header and "dvs_test_cull_order" not in header
    for hook in ("dvs_test_cull_order", "dvs_test_cull_order_device"):
        assert hook + "(" in hook_header and hook in test and hook not in product, hook
    assert "typedef struct dvs_tracker_params" in header and "typedef struct dvs_track_result" in header


def test_null_arguments_are_refused_without_a_device(hiplib):
    from dvslam_amd import tracker as T
    L = T._bind(hiplib)
    r = T.TrackResult()
    img = np.zeros((8, 8), np.uint8); dep = np.zeros((8, 8), np.uint16)
    assert L.dvs_tracker_track(None, img.ctypes.data, 1, 8, dep.ctypes.data, 16, 0, 0, C.byref(r), None, 0) == -6
    assert b"bad argument" in hiplib.dvs_last_error()
    fake = C.c_void_p(1)      # never dereferenced: the result pointer is checked with the handle
    assert L.dvs_tracker_track(fake, img.ctypes.data, 1, 8, dep.ctypes.data, 16, 0, 0, None, None, 0) == -6
    assert L.dvs_tracker_reset(None) == -6 and L.dvs_tracker_synchronize(None) == -6 and L.dvs_tracker_set_stream(None, None) == -6
    n = C.c_int32()
    assert L.dvs_tracker_get_backend_features(None, None, None, None, 0, C.byref(n)) == -6
    h = C.c_void_p()
    assert L.dvs_tracker_create(None, 0, C.byref(h)) == -6 and L.dvs_tracker_create(C.byref(T.default_params()), 0, C.byref(h)) == -6   # rows = cols = 0
    bad = T.default_params(480, 640, 600.0, 600.0, 320.0, 240.0, fm_mode=2)
    assert L.dvs_tracker_create(C.byref(bad), 0, C.byref(h)) == -6 and not h.value
    L.dvs_tracker_destroy(None)


def test_default_params_are_the_references_constants(hiplib):
    from dvslam_amd import tracker as T
    p = T.default_params()
    assert (p.orb.nfeatures, round(p.orb.scale_factor, 6), p.orb.nlevels, p.orb.ini_th_fast, p.orb.min_th_fast) == (1000, 1.2, 8, 20, 7)   # frontend.cpp:206
    assert (round(p.min_depth, 6), p.max_depth, p.max_hamming) == (0.3, 3.0, 50)
    assert (p.fm_threshold, p.fm_confidence, p.fm_max_iters) == (2.0, 0.99, 1000)
    assert (p.cull_max_new, p.cull_min_response) == (200, 50.0)
    assert (p.pnp_iterations, p.pnp_reproj_err, p.pnp_confidence) == (100, 4.0, 0.99)
    assert (p.kf_min_matches, p.kf_max_frames, p.max_translation, p.max_rotation) == (150, 30, 0.5, 0.2)
    assert (p.fm_mode, p.pnp_mode, p.seed_base, p.gray_variant, p.rows, p.cols, p.fx) == (0, 0, 0, 0, 0, 0, 0.0)
    assert C.sizeof(T.TrackerParams) == 200 and C.sizeof(T.TrackResult) == 248        # static_assert'ed in tests/cpp/tracker_adapter.cpp
    import dvslam_amd
    assert dvslam_amd.Tracker is T.Tracker


def test_python_mirror_refuses_bad_frames_before_any_gpu_call():
    from dvslam_amd.tracker import validate_frame
    img = np.zeros((480, 640), np.uint8); dep = np.zeros((480, 640), np.uint16)
    a, b, ch = validate_frame(img, dep, 480, 640)
    assert ch == 1 and a is img and b is dep
    assert validate_frame(np.zeros((480, 640, 3), np.uint8), dep, 480, 640)[2] == 3
    sliced = np.zeros((480, 1280), np.uint8)[:, ::2]
    assert validate_frame(sliced, dep, 480, 640)[0].flags["C_CONTIGUOUS"]
    for bad_img, bad_dep in ((img.astype(np.float32), dep), (img[:100], dep), (np.zeros((480, 640, 4), np.uint8), dep), (img, dep.astype(np.int32)),
                             (img, dep[:, :100]), (np.zeros((2, 480, 640, 3), np.uint8), dep)):
        with pytest.raises(ValueError):
            validate_frame(bad_img, bad_dep, 480, 640)
