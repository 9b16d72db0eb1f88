"""Motion segmentation without a GPU: the C ABI's symbols, argument errors and defaults, the numpy reference's own properties on scene 1
(tests/motion_ref.py), the agreement of its two labellers, and csrc/ccl_union.h — the find / union the kernels run — compiled for the
host into a stand-alone program under AddressSanitizer and UBSan, over the same patterns."""
import ctypes as C
import os
import re
import subprocess
import numpy as np
import pytest
import motion_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["dvs_motion_default_params", "dvs_motion_create", "dvs_motion_destroy", "dvs_motion_set_stream", "dvs_motion_segment_device",
         "dvs_motion_segment", "dvs_tracker_set_motion_mask", "dvs_tracker_get_motion_mask"]
HOOKS = ["dvs_test_motion_label", "dvs_test_motion_stages"]


def _decls(name):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    return set(re.findall(r"\b(dvs_[a-z0-9_]+)\s*\(", text))


def test_symbols_are_declared_and_exported_both_ways(hiplib, hooks):
    assert set(NAMES) <= _decls("dvslam_hip.h")
    assert _decls("dvslam_hip_test_motion.h") == set(HOOKS)
    assert '#include "dvslam_hip_test_motion.h"' in open(os.path.join(ROOT, "include", "dvslam_hip_test.h")).read()
    for n in NAMES:
        assert hasattr(hiplib, n) and hasattr(hooks, n), n
    for n in HOOKS:
        assert hasattr(hooks, n) and not hasattr(hiplib, n), n


def test_struct_sizes_and_defaults(hiplib):
    from dvslam_amd import motion as M
    assert C.sizeof(M.MotionParams) == 72 and C.sizeof(M.MotionStats) == 24
    p = M.default_params()
    assert (p.min_depth_mm, p.max_depth_mm, p.tau0_m, p.tau2_per_m, p.min_area, p.dilate_radius) == (300, 3000, 0.03, 0.005, 200, 8)
    assert (p.rows, p.cols, p.fx, p.fy, p.cx, p.cy) == (0, 0, 0.0, 0.0, 0.0, 0.0)
    assert {k: mr.DEFAULTS[k] for k in mr.DEFAULTS} == {k: getattr(p, k) for k in mr.DEFAULTS}
    # the tracker's structs did not move
    from dvslam_amd import tracker as T
    assert C.sizeof(T.TrackerParams) == 200 and C.sizeof(T.TrackResult) == 248


BAD = [dict(rows=0), dict(rows=4097), dict(cols=0), dict(cols=4097), dict(fx=0.0), dict(fy=-1.0), dict(cx=float("nan")), dict(cy=float("inf")),
       dict(min_depth_mm=-1), dict(min_depth_mm=3000), dict(max_depth_mm=65536), dict(tau0_m=-0.01), dict(tau2_per_m=float("nan")),
       dict(min_area=0), dict(dilate_radius=-1), dict(dilate_radius=32)]


@pytest.mark.parametrize("bad", BAD, ids=lambda d: "%s=%s" % next(iter(d.items())))
def test_argument_errors_come_before_the_device(hiplib, bad):
    from dvslam_amd import motion as M
    M._bind(hiplib)
    h = C.c_void_p()
    good = M.default_params(240, 320, 288.0, 288.0, 159.5, 119.5)
    code = hiplib.dvs_motion_create(C.byref(good), 0, C.byref(h))
    assert code in (0, -5)                        # fine, or no device here: there is no CPU fallback
    if code == 0:
        hiplib.dvs_motion_destroy(h)
    p = M.default_params(240, 320, 288.0, 288.0, 159.5, 119.5)
    for k, v in bad.items():
        setattr(p, k, v)
    assert hiplib.dvs_motion_create(C.byref(p), 0, C.byref(h)) == -6 and not h.value
    assert b"bad argument" in hiplib.dvs_last_error()


def test_null_arguments(hiplib):
    from dvslam_amd import motion as M, tracker as T
    M._bind(hiplib); T._bind(hiplib)
    h = C.c_void_p()
    assert hiplib.dvs_motion_create(None, 0, C.byref(h)) == -6
    assert hiplib.dvs_motion_set_stream(None, None) == -6
    assert hiplib.dvs_motion_segment(None, None, 0, None, 0, None, None, None, 0, None) == -6
    assert hiplib.dvs_motion_segment_device(None, None, 0, None, 0, None, None, None, 0, None) == -6
    assert hiplib.dvs_tracker_set_motion_mask(None, None, 4) == -6
    assert hiplib.dvs_tracker_get_motion_mask(None, None, 0, None, None, None, None) == -6
    hiplib.dvs_motion_destroy(None)


# ---------------------------------------------------------------------------------------------------- the reference's own properties
COLS, ROWS = 320, 240
BOX = (-0.35, -0.15, 0.25, 0.3, 1.0)


@pytest.fixture(scope="module")
def static_scene():
    R, t = mr.SCENE1_MOTION
    return mr.scene1_depth(COLS, ROWS), mr.scene1_depth(COLS, ROWS, R, t)


@pytest.mark.parametrize("axis", ["x", "y", "z"])
@pytest.mark.parametrize("sign", [1, -1])
def test_static_scene_has_no_seeds_with_the_pose_wrong_by_a_third_of_a_degree(static_scene, axis, sign):
    R, t = mr.SCENE1_MOTION
    Dr, Dc = static_scene
    K = mr.scene1_K(COLS, ROWS)
    exact = mr.segment(Dr, Dc, K, R, t)
    assert exact["stats"]["n_seed"] == 0 and exact["stats"]["n_valid"] > 0.9 * COLS * ROWS and (exact["mask"] == 255).all()
    wrong = mr.segment(Dr, Dc, K, mr.rot(axis, 0.3 * sign) @ R, t)
    assert wrong["stats"]["n_seed"] == 0 and wrong["stats"]["n_valid"] > 0.9 * COLS * ROWS


def test_box_displaced_by_more_than_its_width_is_masked_whole():
    R, t = mr.SCENE1_MOTION
    K = mr.scene1_K(COLS, ROWS)
    moved = (BOX[0] + 0.3,) + BOX[1:]
    Dr, Dc = mr.scene1_depth(COLS, ROWS, None, None, BOX), mr.scene1_depth(COLS, ROWS, R, t, moved)
    box = mr.scene1_box_pixels(COLS, ROWS, R, t, moved)
    r = mr.segment(Dr, Dc, K, R, t)
    assert box.sum() > 5000 and (r["mask"][box] == 0).all()          # every box pixel
    assert not (r["seed"] & ~box).any()                               # no seed on a static pixel
    assert r["stats"]["n_components"] == 1 and r["stats"]["n_dynamic"] == box.sum()
    # the rule's known limit: displaced by a third of its width, only the leading part is found
    third = (BOX[0] + BOX[2] / 3,) + BOX[1:]
    Dc3 = mr.scene1_depth(COLS, ROWS, R, t, third)
    box3 = mr.scene1_box_pixels(COLS, ROWS, R, t, third)
    r3 = mr.segment(Dr, Dc3, K, R, t)
    frac = (r3["mask"][box3] == 0).mean()
    assert 0.3 < frac < 0.5 and not (r3["seed"] & ~box3).any(), frac


# ---------------------------------------------------------------------------------------------------- labellers
def _all_patterns():
    for rows, cols in mr.LABEL_SIZES:
        for name, img in mr.patterns(rows, cols):
            yield rows, cols, name, img


def test_the_two_labellers_agree_on_every_pattern():
    n = 0
    for rows, cols, name, img in _all_patterns():
        a, b = mr.labels_scipy(img), mr.labels_union_find(img)
        assert (a == b).all(), (rows, cols, name)
        assert ((a >= 0) == (img != 0)).all()
        roots = a[a >= 0]
        assert (roots <= np.flatnonzero(img.ravel())).all()           # a label is the smallest index of its component
        assert mr.areas(a).sum() == int((img != 0).sum())
        n += 1
    assert n == 5 * 11
    # the patterns are what they say
    by = {nm: im for nm, im in mr.patterns(70, 130)}
    assert len(np.unique(mr.labels_scipy(by["spiral"]))) == 2 and by["spiral"].sum() > 70 * 130 // 3
    assert len(np.unique(mr.labels_scipy(by["comb"]))) == 2 and len(np.unique(mr.labels_scipy(by["comb"][:-1]))) == 66
    assert len(np.unique(mr.labels_scipy(by["diagonal_corner"]))) == 2 and by["diagonal_corner"][31, 31] and by["diagonal_corner"][32, 32]
    assert len(np.unique(mr.labels_scipy(by["every_tile"]))) == 2
    assert len(np.unique(mr.labels_scipy(by["antidiagonals"]))) > 60 and len(np.unique(mr.labels_scipy(by["checkerboard"]))) == 2


def test_ccl_union_header_on_the_host_under_sanitizers(tmp_path):
    """csrc/ccl_union.h in a stand-alone program (tests/cpp/ccl_union_host.cpp), g++ -fsanitize=address,undefined, run directly"""
    exe = os.path.join(str(tmp_path), "ccl_union_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "ccl_union_host.cpp"), "-o", exe])
    cases = list(_all_patterns())
    src, dst = os.path.join(str(tmp_path), "patterns.bin"), os.path.join(str(tmp_path), "labels.bin")
    with open(src, "wb") as fh:
        for rows, cols, _, img in cases:
            fh.write(np.array([rows, cols], np.int32).tobytes()); fh.write(np.ascontiguousarray(img, np.uint8).tobytes())
    out = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == f"{len(cases)} images", out.stdout[-2000:] + out.stderr[-4000:]
    got = np.fromfile(dst, np.int32)
    o = 0
    for rows, cols, name, img in cases:
        n = rows * cols
        lab, area = got[o:o + n].reshape(rows, cols), got[o + n:o + 2 * n].reshape(rows, cols)
        o += 2 * n
        want = mr.labels_scipy(img)
        assert (lab == want).all() and (area == mr.areas(want)).all(), (rows, cols, name)
    assert o == len(got)
