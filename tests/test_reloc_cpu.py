"""Relocalisation without a GPU: the C ABI's symbols, struct sizes against a C99 compile of the header, the adapter header under
-Wall -Werror, argument errors before any device work, and the restatement's own properties (tests/reloc_ref.py): its stages 1-2 against
a second statement with sets and loops, and every condition tests/test_gpu_reloc.py relies on — the share of wrong pairs, the identity
prior that finds nothing, the status each scene ends with, the gate margin of the confirmation, the crafted rows — asserted here from the
restatement alone, so a seed that stops producing a case fails without a GPU.  POSE_MEASURED is measured again with the oracle's statement
of dvs_solve_pnp_ransac and held against its recorded value."""
import ctypes as C
import os
import re
import subprocess
import numpy as np
import pytest
import map_track_ref as mr
import reloc_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "dynamic-visual-slam_amd", "lib")
NAMES = ["dvs_reloc_default_params", "dvs_reloc_create", "dvs_reloc_destroy", "dvs_reloc_set_stream", "dvs_reloc_locate_device", "dvs_reloc_locate",
         "dvs_reloc_get_pairs", "dvs_reloc_set_timing", "dvs_reloc_get_stage_ms", "dvs_backend_relocalize_frame", "dvs_tracker_relocalize"]
HOOKS = ["dvs_test_reloc_landmarks", "dvs_test_reloc_pnp_record"]


def _decls(name):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    return set(re.findall(r"\b(dvs_[a-z0-9_]+)\s*\(", text))


def test_symbols_are_declared_and_exported_both_ways(hiplib, hooks):
    assert set(NAMES) <= _decls("dvslam_hip.h")
    assert {n for n in _decls("dvslam_hip.h") if n.startswith("dvs_reloc_")} == {n for n in NAMES if n.startswith("dvs_reloc_")}
    assert _decls("dvslam_hip_test_reloc.h") == set(HOOKS)
    assert '#include "dvslam_hip_test_reloc.h"' in open(os.path.join(ROOT, "include", "dvslam_hip_test.h")).read()
    assert "dvslam_hip_test_reloc.h" in open(os.path.join(ROOT, "dynamic-visual-slam_amd", "Makefile")).read()
    for n in NAMES:
        assert hasattr(hiplib, n) and hasattr(hooks, n), n
    for n in HOOKS:
        assert hasattr(hooks, n) and not hasattr(hiplib, n), n
    import dvslam_amd
    assert all(hasattr(dvslam_amd, n) for n in ("Relocalizer", "RelocParams", "RelocResult"))
    assert hasattr(dvslam_amd.MappingBackend, "relocalize_frame") and hasattr(dvslam_amd.Tracker, "relocalize")


def test_struct_sizes_match_a_c99_compile_of_the_header(hiplib, tmp_path):
    from dvslam_amd import reloc as RL, map_track as M
    src = os.path.join(str(tmp_path), "sizes.c"); exe = os.path.join(str(tmp_path), "sizes")
    with open(src, "w") as fh:
        fh.write('#include <stdio.h>\n#include <stddef.h>\n#include "dvslam_hip_test.h"\n'
                 'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(dvs_reloc_params), sizeof(dvs_reloc_result),\n'
                 '  sizeof(dvs_reloc_lm_record), offsetof(dvs_reloc_params, pnp_reproj_err), offsetof(dvs_reloc_result, track),\n'
                 '  offsetof(dvs_reloc_result, R), sizeof(dvs_maptrack_result)); return 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), src, "-o", exe])
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [80, 344, 20, 48, 120, 248, 128]
    assert got[1] % 8 == 0
    assert C.sizeof(RL.RelocParams) == 80 and C.sizeof(RL.RelocResult) == 344 and RL.LM_RECORD.itemsize == 20 and rr.LM_RECORD == RL.LM_RECORD
    assert RL.RelocParams.pnp_reproj_err.offset == 48 and RL.RelocResult.track.offset == 120 and RL.RelocResult.R.offset == 248
    assert C.sizeof(M.MapTrackParams) == 232 and C.sizeof(M.MapTrackResult) == 128          # map tracking's structs did not move


def test_defaults_are_the_reference_modules(hiplib):
    from dvslam_amd import reloc as RL
    p = RL.default_params()
    assert {k: getattr(p, k) for k in rr.DEFAULTS} == rr.DEFAULTS
    assert list(p.K4) == [0.0] * 4
    h = C.c_void_p()
    assert RL._bind(hiplib).dvs_reloc_create(C.byref(p), 0, C.byref(h)) == -6 and not h.value       # K4 has no default: zeros are refused


def test_adapter_header_compiles_with_wall_werror(hiplib, tmp_path):
    src = os.path.join(str(tmp_path), "adapter.cpp"); exe = os.path.join(str(tmp_path), "adapter")
    with open(src, "w") as fh:
        fh.write('#include <cstdio>\n#include "dvslam/relocalization.hpp"\n#include "dvslam/map_tracking.hpp"\n'
                 'int main() {\n  dvs_reloc_params p = dvslam::Relocalizer::defaultParams(500.0, 500.0, 320.0, 240.0);\n'
                 '  std::printf("%d %d %g %d\\n", p.max_hamming, p.pnp_iterations, p.K4[2], (int)sizeof(dvs_reloc_result));\n'
                 '  if (dvs_device_count() < 1) return 3;\n'
                 '  dvslam::Relocalizer rl(p);\n  dvslam::Relocalizer::Pairs m = rl.pairs();\n  return m.lm_row.empty() ? 0 : 1;\n}\n')
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), src, "-o", exe, "-L" + LIBDIR,
                           "-ldvslam_hip", "-Wl,-rpath," + LIBDIR, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode in (0, 3) and out.stdout.split() == ["50", "512", "320", "344"], out.stdout[-2000:] + out.stderr[-2000:]


def _good():
    from dvslam_amd import reloc as RL
    return RL.default_params(80.0, 80.0, 50.0, 35.0)


BAD = [dict(fx=0.0), dict(fy=-1.0), dict(cx=float("nan")), dict(cy=float("inf")), dict(max_hamming=-1), dict(max_hamming=258), dict(ratio_pct=100001),
       dict(min_pairs=3), dict(pnp_iterations=0), dict(pnp_iterations=1025), dict(pnp_reproj_err=0.0), dict(pnp_reproj_err=float("nan")),
       dict(pnp_reproj_err=float("inf")), dict(pnp_confidence=0.0), dict(pnp_confidence=1.0), dict(pnp_confidence=float("nan")), dict(min_pnp_inliers=-1),
       dict(min_confirmed=-1)]


@pytest.mark.parametrize("bad", BAD, ids=lambda d: "%s=%s" % next(iter(d.items())))
def test_argument_errors_come_before_the_device(hiplib, bad):
    from dvslam_amd import reloc as RL
    RL._bind(hiplib)
    h = C.c_void_p()
    good = _good()
    code = hiplib.dvs_reloc_create(C.byref(good), 0, C.byref(h))
    assert code in (0, -5)                        # fine, or no device here: there is no CPU fallback
    if code == 0:
        hiplib.dvs_reloc_destroy(h)
    p = _good()
    for k, v in bad.items():
        if k in ("fx", "fy", "cx", "cy"):
            p.K4[("fx", "fy", "cx", "cy").index(k)] = v
        else:
            setattr(p, k, v)
    assert hiplib.dvs_reloc_create(C.byref(p), 0, C.byref(h)) == -6 and not h.value
    assert b"bad argument" in hiplib.dvs_last_error()


def test_null_arguments(hiplib):
    from dvslam_amd import reloc as RL
    RL._bind(hiplib)
    h = C.c_void_p(); n = C.c_int32(); r = RL.RelocResult(); ms = (C.c_double * 3)()
    assert hiplib.dvs_reloc_create(None, 0, C.byref(h)) == -6
    good = _good()
    assert hiplib.dvs_reloc_create(C.byref(good), 0, None) == -6
    assert hiplib.dvs_reloc_set_stream(None, None) == -6
    assert hiplib.dvs_reloc_set_timing(None, 1) == -6
    assert hiplib.dvs_reloc_get_stage_ms(None, ms) == -6
    assert hiplib.dvs_reloc_locate_device(None, None, None, None, None, 0, None, None, 0, C.byref(r)) == -6
    assert hiplib.dvs_reloc_locate(None, None, None, None, None, 0, None, None, 0, C.byref(r)) == -6
    assert hiplib.dvs_reloc_get_pairs(None, 0, None, None, None, None, C.byref(n)) == -6
    assert hiplib.dvs_backend_relocalize_frame(None, None, None, None, None, 0, C.byref(r)) == -6
    assert hiplib.dvs_tracker_relocalize(None, None, None, None, 0, C.byref(r)) == -6
    hiplib.dvs_reloc_destroy(None)
    hiplib.dvs_reloc_default_params(None)


# ---------------------------------------------------------------------------------------------------- the restatement's own properties
SHAPES = [(1, 1), (1, 300), (127, 2), (128, 127), (129, 128), (257, 129), (257, 1), (300, 300)]      # the shapes of test_gpu_reloc.py


def _against_brute(P, xyz, ld, kps, kd):
    st = rr.stages123(P, xyz, ld, kps, kd)
    proposals, kept = rr.brute(P, xyz, ld, kd)
    rec = st["rec"]
    assert {(j, int(rec[j]["best_k"]), int(rec[j]["d_best"])) for j in np.flatnonzero(rec["proposed"])} == proposals
    assert {int(k): (int(j), int(d)) for k, j, d in zip(st["kp_index"], st["lm_row"], st["dist"])} == kept
    assert set(np.flatnonzero(rec["kept"])) == {j for j, _ in kept.values()} and (np.diff(st["kp_index"]) > 0).all()
    return st


@pytest.mark.parametrize("n_lm,n_kp", SHAPES)
@pytest.mark.parametrize("ratio_pct", [75, 0])
def test_stages_1_and_2_equal_the_statement_with_sets_and_loops(n_lm, n_kp, ratio_pct):
    xyz, ld, kps, kd = rr.tie_scene(n_lm, n_kp, 100 * n_lm + n_kp)
    st = _against_brute(rr.params(ratio_pct=ratio_pct), xyz, ld, kps, kd)
    if n_lm >= 127 and n_kp >= 127 and ratio_pct == 0:          # ties decide here: many landmarks share a best distance, keypoints choose
        D = rr.distances(ld, kd)
        assert ((D == D.min(1, keepdims=True)).sum(1) > 1).sum() > n_lm // 2
        assert st["n_proposed"] == n_lm and 5 < st["n_pairs"] < st["n_proposed"]
    if n_kp == 1:
        assert (st["rec"]["d_second"] == -1).all() and st["n_proposed"] >= min(n_lm, 10)


def test_the_crafted_rows_are_what_they_claim():
    P = rr.params()
    xyz, ld, kps, kd, rows = rr.special_scene(P)
    st = _against_brute(P, xyz, ld, kps, kd)
    rec = st["rec"]
    eq, inn = rec[rows["ratio_eq"][0]], rec[rows["ratio_in"][0]]
    assert eq["d_best"] * 100 == P.ratio_pct * eq["d_second"] and not eq["proposed"] and eq["d_best"] < P.max_hamming
    assert inn["d_best"] * 100 < P.ratio_pct * inn["d_second"] and inn["proposed"] and inn["kept"]
    assert rec[rows["at_max_m1"][0]]["d_best"] == P.max_hamming - 1 and rec[rows["at_max_m1"][0]]["proposed"]
    assert rec[rows["at_max"][0]]["d_best"] == P.max_hamming and not rec[rows["at_max"][0]]["proposed"]
    crowd = rec[rows["crowd"]]
    assert len(crowd) == 200 and crowd["proposed"].all() and (crowd["best_k"] == 3).all() and crowd["kept"].sum() == 1
    assert crowd["kept"][1] == 1 and crowd["d_best"][1] == crowd["d_best"].min() == 1 and (crowd["d_best"] == 1).sum() > 10 and crowd["d_best"][0] > 1
    nf = rec[rows["not_finite"]]
    assert (nf["best_k"] == -1).all() and not nf["proposed"].any()
    dup = rec[rows["dup"]]
    assert dup["proposed"].all() and list(dup["kept"]) == [1, 0, 0] and (dup["best_k"] == 4).all()
    fin = xyz.copy(); fin[rows["not_finite"]] = 1.0                       # finite, the first of them (d = 0) would have taken keypoint 4
    assert rr.stages123(P, fin, ld, kps, kd)["rec"][rows["not_finite"][0]]["kept"] == 1
    off = rr.stages123(P.with_(ratio_pct=0), xyz, ld, kps, kd)["rec"]     # ratio_pct <= 0: the equality row proposes too
    assert off[rows["ratio_eq"][0]]["proposed"] and rr.stages123(P.with_(ratio_pct=-5), xyz, ld, kps, kd)["rec"].tobytes() == off.tobytes()


@pytest.fixture(scope="module")
def scene():
    return rr.scene()


@pytest.fixture(scope="module")
def pnp(oracle):
    def run(obj, img, K4, iterations, reproj_err, confidence, seed):
        ok, rvec, tvec, inl, _ = oracle.solve_pnp_ransac(obj, img, K4, iterations, reproj_err, confidence, seed)
        return ok, rvec, tvec, inl
    return run


def test_the_scene_is_what_the_gpu_test_needs(scene):
    s = scene
    ang = np.degrees(np.arccos(np.clip((np.trace(s["R_true"]) - 1) / 2, -1, 1)))
    assert ang > 90 and np.linalg.norm(s["t_true"]) > 1.0 and len(s["xyz"]) == 3000
    st = rr.stages123(s["P"], s["xyz"], s["ldesc"], s["kps"], s["kdesc"])
    wrong = rr.wrong_pairs(s, st)
    print("keypoints", len(s["kps"]), "pairs", st["n_pairs"], "wrong", int(wrong.sum()))
    assert st["n_pairs"] > 250 and 0.30 * st["n_pairs"] <= wrong.sum() <= 0.5 * st["n_pairs"]
    assert (s["kp_truth"] < 0).sum() == 300 and (s["kps"]["x"] % 1 != 0).mean() > 0.9       # distractors; sub-pixel positions
    ident = mr.track(s["MP"], np.eye(3), np.zeros(3), s["xyz"], s["ldesc"], s["kps"], s["kdesc"])
    assert ident["status"] == mr.FEW_MATCHES                    # map tracking alone cannot recover from here
    true = mr.track(s["MP"], s["R_true"], s["t_true"], s["xyz"], s["ldesc"], s["kps"], s["kdesc"])
    assert true["status"] == mr.OK and mr.gate_margin(s["MP"], true) > 1e-6 and true["n_inliers"] >= 100


def test_the_whole_rule_on_the_scene_and_pose_measured(scene, pnp):
    s = scene
    out = rr.locate(s["P"], s["MP"], s["xyz"], s["ldesc"], s["kps"], s["kdesc"], pnp)
    assert out["status"] == rr.OK and out["pnp_success"] == 1 and out["pnp_inliers"] >= 100
    assert not out["pnp_inlier"][rr.wrong_pairs(s, out)].any()                       # RANSAC decided something: no wrong pair is an inlier
    tr = out["track"]
    assert mr.gate_margin(s["MP"], tr) > 1e-6 and tr["n_inliers"] >= s["P"].min_confirmed + 50
    opt = mr.scipy_optimum(s["MP"], tr["Rcw"], tr["tcw"], np.array([[float(v) for v in s["xyz"][j]] for j in tr["kp_lm"][tr["kp_lm"] >= 0]]),
                           np.array([[float(k["x"]), float(k["y"])] for k in s["kps"][tr["kp_lm"] >= 0]]), s["kps"]["octave"][tr["kp_lm"] >= 0], tr["inlier"])
    assert abs(tr["cost"] - opt) <= 1e-6 * opt
    err = max(float(np.abs(out["R"] - s["R_true"]).max()), float(np.abs(out["t"] - s["t_true"]).max()))
    print(f"POSE_MEASURED {err:.3e} (recorded {rr.POSE_MEASURED:.1e})")
    assert 0 < err <= rr.POSE_MEASURED and 10 * rr.POSE_MEASURED <= 1e-2
    # the pose the confirmation starts from is within the window search's reach, and a confirmation asked for more inliers than there are fails
    assert np.abs(out["pnp_t"] - s["t_true"]).max() < 0.02
    more = rr.locate(s["P"].with_(min_confirmed=tr["n_inliers"] + 1), s["MP"], s["xyz"], s["ldesc"], s["kps"], s["kdesc"], pnp)
    assert more["status"] == rr.NOT_CONFIRMED and np.array_equal(more["R"], np.eye(3)) and more["track"]["status"] == mr.OK


def test_rodrigues_pose_is_a_rotation_and_inverts_the_record():
    rng = np.random.default_rng(1)
    for rvec in ([0.0, 0.0, 0.0], [1e-14, 0.0, 0.0], rng.normal(0, 1.5, 3), [0.0, 3.1, 0.0]):
        tvec = rng.normal(0, 2, 3)
        R, t = rr.rodrigues_pose(rvec, tvec)
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-14 and abs(np.linalg.det(R) - 1) < 1e-14
        assert np.abs(R.T @ (np.zeros(3) - t) - tvec).max() < 1e-14                 # the camera centre maps to tvec's origin
        assert np.abs(R.T - mr._exp_so3(list(rvec))).max() < 1e-15


def test_status_paths_of_the_restatement(scene, pnp):
    s = scene
    rnd = rr.random_frame(s)
    o = rr.locate(s["P"], s["MP"], rnd["xyz"], rnd["ldesc"], rnd["kps"], rnd["kdesc"], pnp)
    assert o["status"] == rr.FEW_PAIRS and o["n_pairs"] < s["P"].min_pairs and np.array_equal(o["R"], np.eye(3)) and not o["t"].any()
    cut = rr.cut_to_pairs(s, s["P"].min_pairs - 1)
    o = rr.locate(s["P"], s["MP"], cut["xyz"], cut["ldesc"], cut["kps"], cut["kdesc"], pnp)
    assert o["status"] == rr.FEW_PAIRS and o["n_pairs"] == s["P"].min_pairs - 1
    one_more = rr.cut_to_pairs(s, s["P"].min_pairs)
    assert rr.stages123(s["P"], one_more["xyz"], one_more["ldesc"], one_more["kps"], one_more["kdesc"])["n_pairs"] == s["P"].min_pairs
    bad = rr.all_wrong(s)
    o = rr.locate(s["P"], s["MP"], bad["xyz"], bad["ldesc"], bad["kps"], bad["kdesc"], pnp)
    assert rr.wrong_pairs(bad, o).all() and o["n_pairs"] > 250
    assert o["status"] == rr.NO_POSE and o["pnp_inliers"] < s["P"].min_pnp_inliers // 2      # far below the threshold: no RANSAC variant finds 15
