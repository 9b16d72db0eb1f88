"""Tracking against the map without a GPU: the C ABI's symbols, struct sizes against a C99 compile of the header, the adapter header under
-Wall -Werror, argument errors before any device work, and the numpy reference's own properties (tests/map_track_ref.py): its grid search
against its brute-force search, the true pose on a noise-free scene, and its final cost against scipy.optimize.least_squares.
The last two sections serve tests/test_gpu_map_track_scale.py and tests/test_gpu_map_track_steps.py: every condition those tests rely on
(a scene that really crosses a workgroup, a chunk of the scan, the gate margin of every schedule ...) is asserted here from the reference
alone, so a seed that stops producing the case fails without a GPU; STEP_MEASURED is measured again and held against its recorded value;
and the single-step comparison is shown to notice a wrong Huber weight, a missing sigma2 and a halved term of H."""
import ctypes as C
import os
import re
import subprocess
import numpy as np
import pytest
import map_track_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "dynamic-visual-slam_amd", "lib")
NAMES = ["dvs_maptrack_default_params", "dvs_maptrack_create", "dvs_maptrack_destroy", "dvs_maptrack_set_stream", "dvs_maptrack_search_device",
         "dvs_maptrack_refine_device", "dvs_maptrack_track_device", "dvs_maptrack_track", "dvs_maptrack_get_matches", "dvs_backend_track_frame",
         "dvs_tracker_track_map", "dvs_tracker_get_filtered_features"]
HOOKS = ["dvs_test_maptrack_landmarks", "dvs_test_maptrack_cells", "dvs_test_maptrack_refine_steps"]


def _decls(name):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    return set(re.findall(r"\b(dvs_[a-z0-9_]+)\s*\(", text))


def test_symbols_are_declared_and_exported_both_ways(hiplib, hooks):
    assert set(NAMES) <= _decls("dvslam_hip.h")
    assert {n for n in _decls("dvslam_hip.h") if n.startswith("dvs_maptrack_")} == {n for n in NAMES if n.startswith("dvs_maptrack_")}
    assert _decls("dvslam_hip_test_maptrack.h") == set(HOOKS)
    assert '#include "dvslam_hip_test_maptrack.h"' in open(os.path.join(ROOT, "include", "dvslam_hip_test.h")).read()
    for n in NAMES:
        assert hasattr(hiplib, n) and hasattr(hooks, n), n
    for n in HOOKS:
        assert hasattr(hooks, n) and not hasattr(hiplib, n), n


def test_struct_sizes_match_a_c99_compile_of_the_header(hiplib, tmp_path):
    from dvslam_amd import map_track as M, tracker as T
    src = os.path.join(str(tmp_path), "sizes.c"); exe = os.path.join(str(tmp_path), "sizes")
    with open(src, "w") as fh:
        fh.write('#include <stdio.h>\n#include <stddef.h>\n#include "dvslam_hip_test.h"\n'
                 'int main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(dvs_maptrack_params), sizeof(dvs_maptrack_result),\n'
                 '  sizeof(dvs_maptrack_lm_record), offsetof(dvs_maptrack_params, level_sigma2), offsetof(dvs_maptrack_result, status),\n'
                 '  offsetof(dvs_maptrack_params, chi2_gate)); return 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), src, "-o", exe])
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [232, 128, 40, 104, 104, 80]
    assert C.sizeof(M.MapTrackParams) == 232 and C.sizeof(M.MapTrackResult) == 128 and M.LM_RECORD.itemsize == 40 and mr.LM_RECORD == M.LM_RECORD
    assert M.MapTrackParams.level_sigma2.offset == 104 and M.MapTrackResult.status.offset == 104 and M.MapTrackParams.chi2_gate.offset == 80
    assert C.sizeof(T.TrackerParams) == 200 and C.sizeof(T.TrackResult) == 248          # the tracker's structs did not move


def test_defaults_are_the_reference_modules(hiplib):
    from dvslam_amd import map_track as M
    p = M.default_params()
    assert {k: getattr(p, k) for k in mr.DEFAULTS} == mr.DEFAULTS
    assert (p.rows, p.cols, p.fx, p.fy, p.cx, p.cy) == (0, 0, 0.0, 0.0, 0.0, 0.0)
    assert list(p.level_sigma2) == mr.default_sigma2() + [0.0] * 8
    s = 1.2 ** 2
    assert all(abs(v - s ** i) < 1e-5 * s ** i for i, v in enumerate(mr.default_sigma2()))


def test_adapter_header_compiles_with_wall_werror(hiplib, tmp_path):
    src = os.path.join(str(tmp_path), "adapter.cpp"); exe = os.path.join(str(tmp_path), "adapter")
    with open(src, "w") as fh:
        fh.write('#include <cstdio>\n#include "dvslam/map_tracking.hpp"\n'
                 'int main() {\n  dvs_maptrack_params p = dvslam::MapTracker::defaultParams(480, 640, 500.0, 500.0, 320.0, 240.0);\n'
                 '  std::printf("%d %d %g %d\\n", p.rows, p.cell, p.radius, (int)sizeof(dvs_maptrack_result));\n'
                 '  if (dvs_device_count() < 1) return 3;\n'
                 '  dvslam::MapTracker mt(p);\n  dvslam::MapTracker::Matches m = mt.matches();\n  return m.lm_row.empty() ? 0 : 1;\n}\n')
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), src, "-o", exe, "-L" + LIBDIR,
                           "-ldvslam_hip", "-Wl,-rpath," + LIBDIR, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode in (0, 3) and out.stdout.split() == ["480", "32", "15", "128"], out.stdout[-2000:] + out.stderr[-2000:]


def _good():
    from dvslam_amd import map_track as M
    return M.default_params(70, 100, 80.0, 80.0, 50.0, 35.0)


BAD = [dict(rows=0), dict(rows=16385), dict(cols=0), dict(cols=16385), dict(fx=0.0), dict(fy=-1.0), dict(cx=float("nan")), dict(cy=float("inf")),
       dict(min_z=-0.1), dict(min_z=20.0), dict(max_z=float("inf")), dict(radius=-1.0), dict(radius=float("nan")), dict(cell=0), dict(cell=16385),
       dict(max_hamming=-1), dict(max_hamming=258), dict(ratio_pct=100001), dict(chi2_gate=0.0), dict(chi2_gate=float("nan")), dict(min_matches=2),
       dict(min_inliers=-1), dict(n_levels=0), dict(n_levels=17), dict(sigma2_0=0.0), dict(sigma2_7=float("nan"))]


@pytest.mark.parametrize("bad", BAD, ids=lambda d: "%s=%s" % next(iter(d.items())))
def test_argument_errors_come_before_the_device(hiplib, bad):
    from dvslam_amd import map_track as M
    M._bind(hiplib)
    h = C.c_void_p()
    good = _good()
    code = hiplib.dvs_maptrack_create(C.byref(good), 0, C.byref(h))
    assert code in (0, -5)                        # fine, or no device here: there is no CPU fallback
    if code == 0:
        hiplib.dvs_maptrack_destroy(h)
    p = _good()
    for k, v in bad.items():
        if k.startswith("sigma2_"):
            p.level_sigma2[int(k[7:])] = v
        else:
            setattr(p, k, v)
    assert hiplib.dvs_maptrack_create(C.byref(p), 0, C.byref(h)) == -6 and not h.value
    assert b"bad argument" in hiplib.dvs_last_error()


def test_a_grid_of_more_than_2_to_the_20_cells_is_refused(hiplib):
    from dvslam_amd import map_track as M
    M._bind(hiplib)
    h = C.c_void_p()
    p = M.default_params(16384, 16384, 500.0, 500.0, 8192.0, 8192.0, cell=8)
    assert hiplib.dvs_maptrack_create(C.byref(p), 0, C.byref(h)) == -6
    p.cell = 16
    assert hiplib.dvs_maptrack_create(C.byref(p), 0, C.byref(h)) in (0, -5)
    if h.value:
        hiplib.dvs_maptrack_destroy(h)


def test_null_arguments(hiplib):
    from dvslam_amd import map_track as M
    M._bind(hiplib)
    h = C.c_void_p(); n = C.c_int32(); r = M.MapTrackResult()
    assert hiplib.dvs_maptrack_create(None, 0, C.byref(h)) == -6
    good = _good()
    assert hiplib.dvs_maptrack_create(C.byref(good), 0, None) == -6
    assert hiplib.dvs_maptrack_set_stream(None, None) == -6
    assert hiplib.dvs_maptrack_search_device(None, None, None, None, 0, None, None, 0, None, None, None) == -6
    assert hiplib.dvs_maptrack_refine_device(None, None, None, None, 0, None, None, C.byref(r)) == -6
    assert hiplib.dvs_maptrack_track_device(None, None, None, None, 0, None, None, 0, None, None, C.byref(r)) == -6
    assert hiplib.dvs_maptrack_track(None, None, None, None, 0, None, None, 0, None, None, C.byref(r)) == -6
    assert hiplib.dvs_maptrack_get_matches(None, 0, None, None, None, None, C.byref(n)) == -6
    assert hiplib.dvs_backend_track_frame(None, None, None, None, 0, None, None, C.byref(r)) == -6
    assert hiplib.dvs_tracker_track_map(None, None, None, 0, C.byref(r)) == -6
    assert hiplib.dvs_tracker_get_filtered_features(None, None, None, 0, C.byref(n)) == -6
    hiplib.dvs_maptrack_destroy(None)
    hiplib.dvs_maptrack_default_params(None)


# ---------------------------------------------------------------------------------------------------- the reference's own properties
P_SMALL = mr.Params(70, 100, 80.0, 80.0, 50.0, 35.0)


@pytest.mark.parametrize("n_lm,n_kp,seed", [(257, 300, 3), (65, 70, 4)])
def test_grid_search_equals_brute_force_search_for_every_cell_size(n_lm, n_kp, seed):
    R, t = mr.rot("y", 3.0) @ mr.rot("x", -2.0), np.array([0.05, -0.02, 0.1])
    xyz, ld, kps, kd = mr.search_scene(P_SMALL, n_lm, n_kp, seed, R, t)
    kps["x"][::17] = 100.0                                                       # some keypoints are not binned
    Rcw, tcw = mr.pose_cw(R, t)
    brute = mr.search_brute(P_SMALL, Rcw, tcw, xyz, ld, kps, kd)
    assert brute["visible"].sum() > n_lm // 2 and (brute["d_second"] >= 0).sum() > n_lm // 4
    assert 0 < brute["proposed"].sum() < brute["visible"].sum()
    for cell in (8, 32, 1000):
        grid = mr.search_grid(P_SMALL.with_(cell=cell), Rcw, tcw, xyz, ld, kps, kd)
        assert grid.tobytes() == brute.tobytes(), cell
    lm, dist = mr.assign(brute, n_kp)
    assert brute["kept"].sum() == (lm >= 0).sum() < brute["proposed"].sum()      # some landmarks lost their keypoint
    assert len(set(lm[lm >= 0])) == (lm >= 0).sum()                              # one-to-one
    assert (lm[::17] == -1).all()


def test_bins_are_a_stable_counting_sort():
    xyz, ld, kps, kd = mr.search_scene(P_SMALL, 50, 400, 5)
    start, order, unb = mr.bin_keypoints(P_SMALL, kps)
    assert len(start) == 4 * 3 + 1 and start[-1] == 400 and unb == 0 and sorted(order) == list(range(400))
    for c in range(12):
        seg = order[start[c]:start[c + 1]]
        assert (np.diff(seg) > 0).all()
        assert all((int(kps[k]["y"]) // 32) * 4 + int(kps[k]["x"]) // 32 == c for k in seg)


@pytest.fixture(scope="module")
def noisy():
    """the refinement scene and the reference's result on it; no chi may lie within 1e-6 relative of the gate at any classification, so
    that the GPU's exact flag comparison is never decided by rounding in sin / cos"""
    s = mr.refine_scene()
    r = mr.refine(s["P"], s["R0"], s["t0"], s["X"], s["px"], s["oct"])
    assert len(r["chi_rounds"]) == 4 and mr.gate_margin(s["P"], r) > 1e-6
    return s, r


def test_noise_free_scene_returns_the_true_pose():
    s = mr.refine_scene(outliers=0.0, noise=0.0)
    r = mr.refine(s["P"], s["R0"], s["t0"], s["X"], s["px"], s["oct"])
    assert r["status"] == mr.OK and r["n_inliers"] == 300 and r["cost"] < 1e-18
    assert np.abs(r["R"] - s["R_true"]).max() < 1e-12 and np.abs(r["t"] - s["t_true"]).max() < 1e-11


def test_noisy_scene_ends_at_the_scipy_optimum_of_its_inlier_set(noisy):
    s, r = noisy
    assert r["status"] == mr.OK and not r["inlier"][s["gross"]].any() and r["n_inliers"] > 0.8 * (~s["gross"]).sum()
    ang = np.degrees(np.arccos(np.clip((np.trace(s["R0"].T @ s["R_true"]) - 1) / 2, -1, 1)))
    assert abs(ang - 3.7) < 1e-9 and abs(np.linalg.norm(s["t0"] - s["t_true"]) - 0.07) < 1e-12
    opt = mr.scipy_optimum(s["P"], r["Rcw"], r["tcw"], s["X"], s["px"], s["oct"], r["inlier"])
    assert abs(r["cost"] - opt) <= 1e-6 * opt, (r["cost"], opt)
    assert np.abs(r["R"] - s["R_true"]).max() < 2e-3 and np.abs(r["t"] - s["t_true"]).max() < 1e-2


def test_status_paths_of_the_reference():
    s = mr.refine_scene()
    P = s["P"]
    few = mr.refine(P, s["R0"], s["t0"], s["X"][:14], s["px"][:14], s["oct"][:14])
    assert few["status"] == mr.FEW_MATCHES and few["R"].tobytes() == s["R0"].tobytes() and few["t"].tobytes() == s["t0"].tobytes()
    X = np.repeat(s["X"][:1], 3, 0); px = np.repeat(s["px"][:1], 3, 0)
    deg = mr.refine(P.with_(min_matches=3), s["R0"], s["t0"], X, px, s["oct"][:3])
    assert deg["status"] == mr.DEGENERATE and deg["R"].tobytes() == s["R0"].tobytes()
    g = mr.outlier_scene()
    bad = mr.refine(P, g["R0"], g["t0"], g["X"], g["px"], g["oct"])
    assert g["gross"].all() and bad["status"] == mr.FEW_INLIERS and 3 <= bad["n_inliers"] < P.min_inliers and bad["R"].tobytes() == g["R0"].tobytes()
    assert mr.gate_margin(P, bad) > 1e-6


# ---------------------------------------------------------------------------------------------------- stage 4: schedules, single steps
def _refine(s, *sch, **kw):
    return mr.refine(s["P"], s["R0"], s["t0"], s["X"], s["px"], s["oct"], *sch, **kw)


def _dist(a, b):
    return max(float(np.abs(a["R"] - b["R"]).max()), float(np.abs(a["t"] - b["t"]).max()))


def _lanes(*a):
    return mr.gauss_newton_step(*a, sums="lanes")


@pytest.fixture(scope="module")
def steps():
    """per scene of mr.step_scenes() and schedule: refine() with the float64 step summing by index, summing in lane order, and with the
    longdouble step"""
    return {(k, sch): (_refine(s, *sch), _refine(s, *sch, step=_lanes), _refine(s, *sch, step=mr.gauss_newton_step_ld))
            for k, s in enumerate(mr.step_scenes()) for sch in mr.STEP_SCHEDULES}


def test_every_schedule_ends_ok_with_flags_far_from_the_gate(steps):
    scenes = mr.step_scenes()
    assert [len(s["X"]) for s in scenes] == [300, 257]
    for (k, sch), (a, b, ld) in steps.items():
        P = scenes[k]["P"]
        assert a["status"] == b["status"] == ld["status"] == mr.OK and len(a["chi_rounds"]) == sch[1], (k, sch)
        assert min(mr.gate_margin(P, r) for r in (a, b, ld)) > 1e-6, (k, sch)
        assert (a["inlier"] == ld["inlier"]).all() and (b["inlier"] == ld["inlier"]).all() and P.min_inliers <= a["n_inliers"] < len(a["inlier"])
        assert abs(a["cost"] - ld["cost"]) <= 1e-12 * ld["cost"] and abs(b["cost"] - ld["cost"]) <= 1e-12 * ld["cost"]
    # the first step is a large one, and one step is not the converged pose: what a single step is compared on is not a fixed point
    for k, s in enumerate(scenes):
        one, full = steps[(k, (0, 1, 1))][0], steps[(k, (0, 4, 10))][0]
        assert np.abs(one["R"] - s["R0"]).max() > 1e-2 and _dist(one, full) > 1e-4
        assert steps[(k, (0, 2, 1))][0]["R"].tobytes() == steps[(k, (1, 2, 1))][0]["R"].tobytes()   # rounds 0 and 1 are both robust: the same rule
        assert steps[(k, (0, 4, 10))][0]["R"].tobytes() == _refine(s)["R"].tobytes()


def test_step_measured_is_not_below_what_is_measured_here(steps):
    worst = max(max(_dist(a, ld), _dist(b, ld)) for a, b, ld in steps.values())
    print(f"STEP_MEASURED {worst:.3e} (recorded {mr.STEP_MEASURED:.1e})")
    assert 0 < worst <= mr.STEP_MEASURED
    assert 10 * mr.STEP_MEASURED <= 1e-9          # the bound the device's single steps are held to may not exceed the full run's tolerance


@pytest.mark.parametrize("mutate", mr.MUTATIONS)
def test_a_single_step_shows_a_wrong_weight_a_missing_sigma_and_a_halved_term(steps, mutate):
    """a converged run forgets these (a wrong Huber weight moves the final pose by 1e-15); one step does not"""
    schedules = [(0, 1, 1)] if mutate.startswith("w_") else [(0, 1, 1), (2, 1, 1)]     # the Huber weight exists in the robust rounds only
    for k, s in enumerate(mr.step_scenes()):
        for sch in schedules:
            wrong = _refine(s, *sch, step=lambda *a: mr.gauss_newton_step(*a, mutate=mutate))
            d = float(np.abs(wrong["R"] - steps[(k, sch)][0]["R"]).max())
            print(mutate, len(s["X"]), sch, f"{d:.2e}")
            assert wrong["status"] in (mr.OK, mr.FEW_INLIERS) and d > 1000 * 10 * mr.STEP_MEASURED and d > 1e-4


REFINE_SIZES = [15, 63, 64, 65, 255, 256, 257, 513, 1000]


def test_refine_sizes_end_ok_with_flags_far_from_the_gate():
    margins = {}
    for n in REFINE_SIZES:
        s = mr.refine_scene(n=n, seed=7)
        r = _refine(s)
        assert r["status"] == mr.OK and len(r["inlier"]) == n, n
        margins[n] = mr.gate_margin(s["P"], r)
    print(margins)
    assert min(margins.values()) > 1e-6


def test_pairs_behind_the_camera_and_outside_the_octave_table_add_nothing():
    s, behind, badoct = mr.pair_rule_scene()
    both = np.r_[behind, badoct]
    Rcw, tcw = mr.pose_cw(s["R_true"], s["t_true"])
    assert all(-4.0 <= mr.camera_point(Rcw, tcw, s["X"][i])[2] <= -0.5 for i in behind)
    r = _refine(s)
    assert r["status"] == mr.OK and r["n_inliers"] == 248 and mr.gate_margin(s["P"], r) > 1e-6 and not r["inlier"][both].any()
    assert all(np.isinf(c[both]).all() for c in r["chi_rounds"])
    d = dict(s, X=np.delete(s["X"], both, 0), px=np.delete(s["px"], both, 0), oct=np.delete(s["oct"], both))
    r0 = _refine(d)
    assert r0["R"].tobytes() == r["R"].tobytes() and r0["t"].tobytes() == r["t"].tobytes() and r0["cost"] == r["cost"]
    assert (np.delete(r["inlier"], both) == r0["inlier"]).all()
    P3 = s["P"].with_(n_levels=3, level_sigma2=s["P"].level_sigma2[:3])                                   # a shorter table: every pair of octave >= 3 goes the same way
    r3 = mr.refine(P3, s["R0"], s["t0"], s["X"], s["px"], s["oct"])
    high = s["oct"] >= 3
    assert r3["status"] == mr.OK and mr.gate_margin(P3, r3) > 1e-6 and high.sum() > 150 and not r3["inlier"][high].any() and r3["n_inliers"] > 50


def test_a_pair_behind_the_camera_at_the_prior_comes_in_front_and_ends_an_inlier():
    s, i = mr.crossing_scene()
    Rp, tp = mr.pose_cw(s["R0"], s["t0"])
    Rt, tt = mr.pose_cw(s["R_true"], s["t_true"])
    assert mr.camera_point(Rp, tp, s["X"][i])[2] < -0.01 and abs(mr.camera_point(Rt, tt, s["X"][i])[2] - 0.02) < 1e-12
    r = _refine(s)
    assert r["status"] == mr.OK and r["inlier"][i] == 1 and mr.gate_margin(s["P"], r) > 1e-6 and all(np.isfinite(c[i]) for c in r["chi_rounds"])
    one = _refine(s, 0, 1, 1)                                       # the first step's sums run without it
    d = dict(s, X=np.delete(s["X"], i, 0), px=np.delete(s["px"], i, 0), oct=np.delete(s["oct"], i))
    assert one["Rcw"] == _refine(d, 0, 1, 1)["Rcw"]


def test_pairs_that_are_not_finite():
    """a pixel that is not finite ends the refinement; a position that is not finite is a permanent outlier"""
    s = mr.refine_scene()
    base = _refine(s)
    for bad in (np.nan, np.inf, -np.inf):
        px = s["px"].copy(); px[11, 1] = bad
        r = _refine(dict(s, px=px))
        assert r["status"] == mr.DEGENERATE and r["R"].tobytes() == s["R0"].tobytes() and r["t"].tobytes() == s["t0"].tobytes()
        assert not r["inlier"].any() and r["cost"] == 0.0 and r["n_inliers"] == 0
    rows = [11, 12, 13]
    X = s["X"].copy(); X[11, 0] = np.nan; X[12, 1] = np.inf; X[13] = -np.inf
    r = _refine(dict(s, X=X))
    r0 = _refine(dict(s, X=np.delete(s["X"], rows, 0), px=np.delete(s["px"], rows, 0), oct=np.delete(s["oct"], rows)))
    assert base["inlier"][rows].all()                               # they would have been inliers
    assert r["status"] == mr.OK and not r["inlier"][rows].any() and r["R"].tobytes() == r0["R"].tobytes() and r["cost"] == r0["cost"]
    # a pixel that is not finite on a pair that never enters a sum ends nothing
    px = s["px"].copy(); px[11] = np.nan
    r = _refine(dict(s, X=X, px=px))
    assert r["status"] == mr.OK and r["R"].tobytes() == r0["R"].tobytes()


def test_the_thousand_landmark_frame_fills_four_chunks_of_the_gather():
    t = mr.track_scene(n=1000)
    w = mr.track(t["P"], t["R0"], t["t0"], t["xyz"], t["ldesc"], t["kps"], t["kdesc"])
    assert len(t["kps"]) == 963 and w["n_matches"] == 949 and w["status"] == mr.OK and mr.gate_margin(t["P"], w) > 1e-6
    assert [int((w["kp_lm"][c:c + 256] >= 0).sum()) for c in range(0, 963, 256)] == [251, 254, 253, 191]
    assert (w["inlier"] == 0).sum() > 50


# ---------------------------------------------------------------------------------------------------- stages 1-3 at frame structure
FRAME_COUNTS = [(1000, 255), (1000, 256), (1000, 257), (1000, 513), (3000, 2000)]
FRAME_GRIDS = [(512, 512, 32, 256), (1, 257, 1, 257), (480, 640, 32, 300), (480, 640, 16, 1200), (480, 640, 8, 4800)]    # rows, cols, cell, cells


def _search(P, xyz, ld, kps, kd, R=mr.FRAME_R, t=mr.FRAME_T):
    Rcw, tcw = mr.pose_cw(R, t)
    rec = mr.search_grid(P, Rcw, tcw, xyz, ld, kps, kd)
    lm, _ = mr.assign(rec, len(kps))
    return rec, lm


@pytest.mark.parametrize("n_lm,n_kp", FRAME_COUNTS)
def test_frame_scenes_propose_and_keep_enough(n_lm, n_kp):
    P = mr.frame_params()
    xyz, ld, kps, kd, ids = mr.frame_scene(P, n_lm, n_kp)
    rec, lm = _search(P, xyz, ld, kps, kd)
    print(n_lm, n_kp, "proposed", rec["proposed"].sum(), "kept", (lm >= 0).sum())
    assert rec["proposed"].sum() > 100 and (lm >= 0).sum() > 100 and (np.diff(ids) > 0).all() and ids[0] > n_lm
    if n_kp == 2000:
        assert (lm >= 0).sum() < rec["proposed"].sum() - 100


@pytest.mark.parametrize("rows,cols,cell,ncell", FRAME_GRIDS)
def test_every_chunk_of_the_scan_holds_keypoints(rows, cols, cell, ncell):
    P = mr.frame_params(cell=cell).with_(rows=rows, cols=cols)
    xyz, ld, kps, kd, _ = mr.frame_scene(P, 1000, 513)
    start, order, unb = mr.bin_keypoints(P, kps)
    assert len(start) == ncell + 1 and unb == 0
    chunks = [int(start[min(c + 256, ncell)] - start[c]) for c in range(0, ncell, 256)]
    print(chunks)
    assert len(chunks) == (ncell + 255) // 256 and min(chunks) > 0


def test_the_dense_cell_spans_workgroups_and_the_order_is_not_the_index_order():
    P = mr.small_params()
    for n_before in (0, 200):
        xyz, ld, kps, kd, cell = mr.dense_cell_scene(P, n_before)
        start, order, unb = mr.bin_keypoints(P, kps)
        assert (start[cell], start[cell + 1]) == (n_before, n_before + 300) and unb == 0
        assert (order != np.arange(len(order))).any() and (np.diff(order[start[cell]:start[cell + 1]]) > 0).all()
        if n_before:
            assert start[cell] < 255 and start[cell + 1] > 257                          # the segment straddles two workgroups of k_mt_order
        rec, lm = _search(P, xyz, ld, kps, kd, np.eye(3), np.zeros(3))
        assert (rec["d_second"] >= 0).sum() > 50 and (lm >= 0).sum() > 10


def test_the_crowded_scene_makes_keypoints_choose():
    P = mr.frame_params()
    xyz, ld, kps, kd, ids = mr.crowded_scene(P)
    rec, lm = _search(P, xyz, ld, kps, kd)
    n = mr.proposals_per_keypoint(rec, len(kps))
    print("matched", (lm >= 0).sum(), "with two or more proposals", (n[lm >= 0] >= 2).sum(), "most", n.max())
    assert len(xyz) == 20000 and len(kps) == 2000 and (lm >= 0).sum() > 1000 and 2 * (n[lm >= 0] >= 2).sum() >= (lm >= 0).sum()
