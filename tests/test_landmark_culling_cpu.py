"""Landmark culling without a GPU (include/dvslam_hip.h "Landmark culling"): the symbols declared and exported, the header as C99 with the
struct sizes the ctypes mirrors have, the argument errors that need no handle, the C++ adapter under plain g++, the restatement
(tests/landmark_culling_ref.py) against a brute-force triple loop and a case worked out by hand, and the conditions the scenes of
tests/test_gpu_landmark_culling.py must meet, asserted on the restatement and map_track_ref alone."""
import ctypes as C
import os
import re
import subprocess
import numpy as np
import pytest
import backend_ref as br
import landmark_culling_ref as lcr
import loop_closing_ref as lc
import map_track_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "dynamic-visual-slam_amd", "lib")
NAMES = ["dvs_lm_cull_default_params", "dvs_backend_set_tracking_stats", "dvs_backend_cull_landmarks", "dvs_backend_get_landmark_stats",
         "dvs_backend_set_landmark_stats", "dvs_backend_clear_landmark_stats"]


def test_symbols_declared_and_exported(hiplib, hooks):
    """fails without the feature (no such symbols)"""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dvslam_hip.h")).read(), flags=re.S)
    decl = set(re.findall(r"\b(dvs_[a-z0-9_]+)\s*\(", text))
    assert set(NAMES) <= decl
    for n in NAMES:
        assert hasattr(hiplib, n) and hasattr(hooks, n), n
    exported = subprocess.run(["nm", "-D", "--defined-only", os.path.join(LIBDIR, "libdvslam_hip.so")], capture_output=True, text=True, check=True).stdout
    for n in NAMES:
        assert f" T {n}\n" in exported, n
    assert not any(n.startswith(("dvs_maptrack_", "dvs_covis_", "dvs_fuse_", "dvs_reloc_")) for n in NAMES)


def test_header_is_c99_and_the_structs_match_their_mirrors(hiplib, tmp_path):
    from dvslam_amd import backend as B
    src = os.path.join(str(tmp_path), "sizes.c"); exe = os.path.join(str(tmp_path), "sizes")
    with open(src, "w") as fh:
        fh.write('#include <stdio.h>\n#include <stddef.h>\n#include "dvslam_hip.h"\n'
                 'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(dvs_lm_cull_params), offsetof(dvs_lm_cull_params, min_visible),\n'
                 '  offsetof(dvs_lm_cull_params, weak_age_kf), offsetof(dvs_lm_cull_params, weak_max_views), sizeof(dvs_lm_cull_result),\n'
                 '  offsetof(dvs_lm_cull_result, n_by_ratio), offsetof(dvs_lm_cull_result, n_weak), offsetof(dvs_lm_cull_result, n_landmarks_removed),\n'
                 '  offsetof(dvs_lm_cull_result, n_keyframes_touched), offsetof(dvs_lm_cull_result, reserved));\n  return 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), src, "-o", exe])
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [16, 4, 8, 12, 32, 4, 8, 12, 20, 24]
    P, R = B.LmCullParams, B.LmCullResult
    assert [C.sizeof(P), P.min_visible.offset, P.weak_age_kf.offset, P.weak_max_views.offset, C.sizeof(R), R.n_by_ratio.offset, R.n_weak.offset,
            R.n_landmarks_removed.offset, R.n_keyframes_touched.offset, R.reserved.offset] == got
    p = B.lm_cull_params()
    assert {k: getattr(p, k) for k in lcr.DEFAULTS} == lcr.DEFAULTS
    q = B.lm_cull_params(found_ratio_pct=0, weak_age_kf=-1, min_visible=7, weak_max_views=3)
    assert (q.found_ratio_pct, q.min_visible, q.weak_age_kf, q.weak_max_views) == (0, 7, -1, 3)
    for bad in (dict(min_visibel=3), dict(reserved=1)):
        with pytest.raises(TypeError):
            B.lm_cull_params(**bad)


def test_null_and_range_errors_come_before_any_handle_work(hiplib):
    from dvslam_amd import backend as B
    B._bind(hiplib)
    n, r, nf = C.c_int32(), B.LmCullResult(), C.c_int64()
    hiplib.dvs_lm_cull_default_params(None)
    assert hiplib.dvs_backend_cull_landmarks(None, None, 0, C.byref(r), 0, None, None, C.byref(n)) == -6
    assert b"bad argument" in hiplib.dvs_last_error()
    assert hiplib.dvs_backend_set_tracking_stats(None, 1) == -6
    assert hiplib.dvs_backend_clear_landmark_stats(None) == -6
    assert hiplib.dvs_backend_get_landmark_stats(None, 0, None, None, None, None, None, C.byref(n), C.byref(nf)) == -6
    assert hiplib.dvs_backend_set_landmark_stats(None, 0, None, None, None) == -6
    # the parameters are judged before the handle is read: any non-null address does for one
    fake = C.create_string_buffer(64)
    h = C.cast(fake, C.c_void_p)
    assert hiplib.dvs_backend_cull_landmarks(h, None, 0, C.byref(r), 0, None, None, None) == -6              # no n_culled
    assert hiplib.dvs_backend_cull_landmarks(h, None, 0, C.byref(r), -1, None, None, C.byref(n)) == -6       # cap < 0
    for bad in (dict(found_ratio_pct=101), dict(min_visible=0), dict(min_visible=-3), dict(weak_max_views=-1)):
        n.value = 77
        assert hiplib.dvs_backend_cull_landmarks(h, C.byref(B.lm_cull_params(**bad)), 1, C.byref(r), 0, None, None, C.byref(n)) == -6, bad
        assert b"bad argument" in hiplib.dvs_last_error() and n.value == 0
    assert hiplib.dvs_backend_get_landmark_stats(h, 0, None, None, None, None, None, None, None) == -6       # no n
    assert hiplib.dvs_backend_get_landmark_stats(h, -1, None, None, None, None, None, C.byref(n), None) == -6
    assert hiplib.dvs_backend_set_landmark_stats(h, -1, None, None, None) == -6
    assert hiplib.dvs_backend_set_landmark_stats(h, 2, None, None, None) == -6                                # rows announced, none given
    ids = np.array([5, 5], np.uint64); one = np.array([1, 1], np.int32); two = np.array([2, 2], np.int32); neg = np.array([-1, -1], np.int32)
    ok = np.array([5, 6], np.uint64)
    assert hiplib.dvs_backend_set_landmark_stats(h, 2, ids.ctypes.data, one.ctypes.data, one.ctypes.data) == -6       # ids do not ascend strictly
    assert hiplib.dvs_backend_set_landmark_stats(h, 2, ok.ctypes.data, one.ctypes.data, two.ctypes.data) == -6        # found > visible
    assert hiplib.dvs_backend_set_landmark_stats(h, 2, ok.ctypes.data, neg.ctypes.data, neg.ctypes.data) == -6        # negative
    assert fake.raw == bytes(64)


def test_adapter_header_compiles_with_plain_gpp(hiplib, tmp_path):
    src = os.path.join(str(tmp_path), "adapter.cpp"); exe = os.path.join(str(tmp_path), "adapter")
    with open(src, "w") as fh:
        fh.write('#include <cstdio>\n#include "dvslam/landmark_culling.hpp"\n'
                 'int main() {\n  dvslam::LandmarkCullParams p;\n'
                 '  std::printf("%d %d %d %d %d %d\\n", p.found_ratio_pct, p.min_visible, p.weak_age_kf, p.weak_max_views, (int)sizeof(dvs_lm_cull_params), (int)sizeof(dvs_lm_cull_result));\n'
                 '  if (dvs_device_count() < 1) return 3;\n'
                 '  dvs_backend_params bp; dvs_backend_default_params(&bp); bp.fx = bp.fy = 500.0; bp.cx = 320.0; bp.cy = 240.0;\n'
                 '  dvslam::MappingBackend map(bp);\n  dvslam::setTrackingStats(map, true);\n  dvslam::LandmarkCullReport r = dvslam::cullLandmarks(map, p);\n'
                 '  dvslam::LandmarkStats s = dvslam::landmarkStats(map);\n  dvslam::setLandmarkStats(map, {}, {}, {});\n  dvslam::clearLandmarkStats(map);\n'
                 '  if (r.result.n_landmarks != 0 || !r.culled_id.empty() || !s.id.empty() || s.n_frames_recorded != 0) return 1;\n'
                 '  p.min_visible = 0;\n  try { dvslam::cullLandmarks(map, p); } catch (const std::runtime_error&) { return 0; }\n'
                 '  return 1;\n}\n')
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), src, "-o", exe, "-L" + LIBDIR,
                           "-ldvslam_hip", "-Wl,-rpath," + LIBDIR, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode in (0, 3) and out.stdout.split() == ["25", "4", "2", "1", "16", "32"], out.stdout[-2000:] + out.stderr[-2000:]


# ---------------------------------------------------------------------------------------------------- the restatement
def _ref(keyframes):
    ref = br.BackendRef(br.FX, br.FY, br.CX, br.CY, filtered=(br.PERSON,))
    for kf in keyframes:
        lc.add(ref, kf)
    return ref


def _hand_ref():
    """keyframes 10, 11, 12, 13 (indices 0..3); frame 99 is no keyframe.  Landmark 1: rows of 10, 11 -> n 2, first kf 0, age 3.  Landmark 2: one
    row of 12 -> n 1, age 1.  Landmark 3: a row of frame 99, then one of 11 -> n 2, the first VALID view is 11: age 2.  Landmark 4: a row of
    frame 99 only -> n 1, age -1.  Landmark 5: no row -> n 0, age -1.  Landmark 6: one row of 10 -> n 1, age 3."""
    ref = br.BackendRef(br.FX, br.FY, br.CX, br.CY)
    z = np.zeros(32, np.uint8)
    for f in (10, 11, 12, 13):
        ref.kfs.append(dict(frame=f, R=np.eye(3).reshape(9), t=np.zeros(3), stamp=f, obs_ids=[]))
    rows = [(10, 1), (99, 3), (11, 1), (12, 2), (99, 4), (11, 3), (10, 6)]
    for i, (f, l) in enumerate(rows):
        ref.obs.append(dict(id=100 + i, frame=f, px=np.zeros(2, np.float32), desc=z, cls=0, lm=l))
        for kf in ref.kfs:
            if kf["frame"] == f:
                kf["obs_ids"].append(100 + i)
    for l in (1, 2, 3, 4, 5, 6):
        ref.db.setdefault(0, {})[l] = dict(id=l, cls=0, pos=np.zeros(3, np.float32), desc=z, obs_ids=[o["id"] for o in ref.obs if o["lm"] == l], count=1, last_seen=0)
    ref.next_obs, ref.next_lm = 107, 7
    return ref


def test_decide_and_apply_by_hand():
    ref = _hand_ref()
    assert lcr.views(ref) == {1: (2, 3), 2: (1, 1), 3: (2, 2), 4: (1, -1), 5: (0, -1), 6: (1, 3)}
    # defaults: F needs visible >= 4 and found * 100 < 25 * visible; W needs age >= 2 and n <= 1
    stats = {1: [8, 2], 2: [8, 1], 3: [3, 0], 6: [4, 0], 77: [9, 9]}
    ids, why, res = lcr.decide(ref, stats)
    assert (ids, why) == ([2, 6], [1, 1]) and res == dict(n_landmarks=6, n_by_ratio=2, n_weak=0)       # 1: 200 < 200 is false; 3: too few frames; 6: F before W
    ids, why, res = lcr.decide(ref, {})
    assert (ids, why) == ([6], [2])                                                                     # 4 and 5 are old by no view at all: never weak
    assert lcr.decide(ref, {}, weak_age_kf=1)[0] == [2, 6] and lcr.decide(ref, {}, weak_age_kf=1, weak_max_views=2)[0] == [1, 2, 3, 6]
    assert lcr.decide(ref, {}, weak_age_kf=3, weak_max_views=2)[0] == [1, 6] and lcr.decide(ref, {}, weak_age_kf=4, weak_max_views=2)[0] == []
    assert lcr.decide(ref, stats, found_ratio_pct=0, weak_age_kf=-1)[0] == []
    assert lcr.decide(ref, stats, found_ratio_pct=26, weak_age_kf=-1)[0] == [1, 2, 6]
    assert lcr.decide(ref, stats, min_visible=3, weak_age_kf=-1)[0] == [2, 3, 6]
    for bad in (dict(found_ratio_pct=101), dict(min_visible=0), dict(weak_max_views=-1)):
        with pytest.raises(ValueError):
            lcr.decide(ref, stats, **bad)
    out = lcr.cull(ref, stats, weak_age_kf=3, weak_max_views=2)                                        # F: 2, 6; W: 1
    assert out["culled_id"].tolist() == [1, 2, 6] and out["culled_reason"].tolist() == [2, 1, 1]
    assert (out["n_landmarks_removed"], out["n_observations_removed"], out["n_keyframes_touched"]) == (3, 4, 3)
    assert [o["id"] for o in ref.obs] == [101, 104, 105] and [kf["obs_ids"] for kf in ref.kfs] == [[], [105], [], []]
    assert stats == {3: [3, 0], 77: [9, 9]} and lcr.align(ref, stats) == {3: [3, 0], 4: [0, 0], 5: [0, 0]}


def test_decide_equals_a_brute_force_triple_loop():
    """for every landmark, for every observation row, for every keyframe: no index, no dict of views"""
    rng = np.random.default_rng(5)
    ref = _ref(br.make_scene(nkf=6, npoints=120))
    ref.kfs.pop(2)                                                            # rows whose frame is no keyframe any more
    L = lcr.landmarks(ref)
    stats = {lid: [int(v), int(rng.integers(0, v + 1))] for lid, v in zip(L, rng.integers(0, 12, len(L)))}
    for params in (dict(), dict(weak_age_kf=0), dict(found_ratio_pct=50, min_visible=1, weak_age_kf=3, weak_max_views=2), dict(found_ratio_pct=0), dict(weak_age_kf=-1),
                   dict(found_ratio_pct=100, min_visible=2, weak_age_kf=4, weak_max_views=0)):
        P = dict(lcr.DEFAULTS, **params)
        want = []
        for lid in sorted(L):
            n, first = 0, None
            for o in ref.obs:
                if o["lm"] != lid:
                    continue
                n += 1
                for k in range(len(ref.kfs)):
                    if ref.kfs[k]["frame"] == o["frame"] and first is None:
                        first = k
            age = len(ref.kfs) - 1 - first if first is not None else -1
            v, f = stats[lid]
            if P["found_ratio_pct"] > 0 and v >= P["min_visible"] and 100 * f < P["found_ratio_pct"] * v:
                want.append((lid, 1))
            elif P["weak_age_kf"] >= 0 and age >= P["weak_age_kf"] and n <= P["weak_max_views"]:
                want.append((lid, 2))
        ids, why, res = lcr.decide(ref, stats, **params)
        assert list(zip(ids, why)) == want and res["n_by_ratio"] + res["n_weak"] == len(want), params
    assert any(a == -1 for _, a in lcr.views(ref).values()) and len({a for _, a in lcr.views(ref).values()}) >= 5


def test_record_by_hand():
    stats = {1: [0, 0], 2: [3, 1], 3: [lcr.INT32_MAX, 7], 4: [5, 5]}
    before = {k: list(v) for k, v in stats.items()}
    args = ([1, 2, 3, 4, 9], [1, 1, 1, 0, 1], [2, -1, 3, 1, 4], [1, 1, 1, 0, 1])     # keypoint 3 kept landmark 1 as an outlier; landmark 4 is kept, not visible: impossible, ignored
    for status in (mr.FEW_MATCHES, mr.FEW_INLIERS, mr.DEGENERATE):
        lcr.record(stats, *args, status)
        assert stats == before
    lcr.record(stats, *args, mr.OK)
    assert stats == {1: [1, 0], 2: [4, 2], 3: [lcr.INT32_MAX, 7], 4: [5, 5]}


# ---------------------------------------------------------------------------------------------------- the scenes
@pytest.mark.parametrize("n_lm", [255, 256, 257, 513])
def test_the_recording_scene_meets_its_conditions(n_lm):
    S = lcr.record_scene(n_lm)
    P = lcr.track_params()
    ref = _ref([S["kf"]])
    L = ref.landmark_table()
    kind = S["kind"]
    assert len(L["id"]) == n_lm and {(kind == k).sum() > 60 for k in range(3)} == {True}
    bits = np.unpackbits(S["kf"]["desc"], axis=1).astype(np.int32)
    H = bits @ (1 - bits).T + (1 - bits) @ bits.T
    assert H[~np.eye(n_lm, dtype=bool)].min() > P.max_hamming + 30                       # unrelated descriptors: far above max_hamming
    out = mr.track(P, S["R"], S["t"], L["xyz"], L["desc"], S["kps"], S["kdesc"])
    rec = out["rec"]
    uv = np.stack([rec["u"], rec["v"]], 1)[kind != lcr.KIND_C]
    d = np.abs(uv[:, None, :] - uv[None, :, :]).max(2)
    assert d[~np.eye(len(uv), dtype=bool)].min() > 2 * P.radius                         # projections more than 2 * radius apart
    assert rec["visible"][kind != lcr.KIND_C].all() and not rec["visible"][kind == lcr.KIND_C].any()
    assert rec["kept"][kind == lcr.KIND_A].all() and not rec["proposed"][kind != lcr.KIND_A].any() and (rec["d_best"][kind == lcr.KIND_B] == -1).all()
    true_kp = np.zeros(len(S["kps"]), bool); true_kp[S["true_kp"]] = True
    assert out["status"] == mr.OK and (out["kp_lm"] >= 0).tolist() == true_kp.tolist() and out["kp_inlier"][true_kp].all()     # every A pair an inlier, no decoy kept
    stats = lcr.align(ref, {})
    kp_id = np.where(out["kp_lm"] >= 0, L["id"][np.maximum(out["kp_lm"], 0)].astype(np.int64), -1)
    lcr.record(stats, L["id"], rec["visible"], kp_id, out["kp_inlier"], out["status"])
    tab = lcr.stats_table(ref, stats)
    for k, want in ((lcr.KIND_A, (1, 1)), (lcr.KIND_B, (1, 0)), (lcr.KIND_C, (0, 0))):
        assert (tab["visible"][kind == k] == want[0]).all() and (tab["found"][kind == k] == want[1]).all()
    # the two refused frames
    few = mr.track(P, S["R"], S["t"], L["xyz"], L["desc"], S["kps"][:6], S["kdesc"][:6])
    assert few["status"] == mr.FEW_MATCHES
    off = mr.track(P, S["R"], S["t_moved"], L["xyz"], L["desc"], S["kps"], S["kdesc"])
    assert off["status"] == mr.FEW_INLIERS and (off["kp_lm"] >= 0).sum() == lcr.N_DECOYS >= P.min_matches and 3 <= off["n_inliers"] <= 7 < P.min_inliers
    assert not (off["kp_lm"] >= 0)[true_kp].any() and off["rec"]["visible"].sum() == (kind != lcr.KIND_C).sum()


def test_the_object_scene_meets_its_conditions():
    kfs, q = lcr.object_scene()
    P = lcr.track_params()
    ref = _ref(kfs)
    assert ref.ties == 0
    L = ref.landmark_table()
    obj = lcr.object_ids(ref, q)
    assert len(L["id"]) == lcr.STATIC_N + lcr.OBJECT_N and len(obj) == lcr.OBJECT_N >= 30
    assert all(v == (lcr.OBJECT_NKF, lcr.OBJECT_NKF - 1) for v in lcr.views(ref).values())       # at least two views each: W cannot fire
    out = mr.track(P, q["R"], q["t"], L["xyz"], L["desc"], q["kps"], q["kdesc"])
    assert out["status"] == mr.OK and out["n_visible"] == len(L["id"]) and out["n_inliers"] == lcr.STATIC_N
    stats = lcr.align(ref, {})
    kp_id = np.where(out["kp_lm"] >= 0, L["id"][np.maximum(out["kp_lm"], 0)].astype(np.int64), -1)
    for _ in range(lcr.DEFAULTS["min_visible"]):
        lcr.record(stats, L["id"], out["rec"]["visible"], kp_id, out["kp_inlier"], out["status"])
    ids, why, res = lcr.decide(ref, stats)
    assert set(ids) == obj and set(why) == {lcr.REASON_F} and res == dict(n_landmarks=len(L["id"]), n_by_ratio=lcr.OBJECT_N, n_weak=0)
    static = set(lcr.landmarks(ref)) - obj
    assert all(lcr.rule(*stats[i], *lcr.views(ref)[i], lcr.DEFAULTS) == 0 for i in static)       # zero static landmarks in either rule
    rep = lcr.cull(ref, stats)
    assert rep["n_observations_removed"] == lcr.OBJECT_N * lcr.OBJECT_NKF and rep["n_keyframes_touched"] == lcr.OBJECT_NKF
    after = ref.landmark_table()
    out2 = mr.track(P, q["R"], q["t"], after["xyz"], after["desc"], q["kps"], q["kdesc"])
    assert out2["n_visible"] == out["n_visible"] - lcr.OBJECT_N and out2["status"] == mr.OK


def test_the_apply_scene_fills_more_than_two_blocks_of_the_compaction():
    """test_gpu_landmark_culling.py's "block" case takes ids[256:512] out: rows must stay on both sides, the later ones in a third 256-row block"""
    from test_gpu_landmark_culling import BIG_SCENE
    ref = _ref(br.make_scene(**BIG_SCENE)[:3])
    assert len(ref.landmark_table()["id"]) >= 513 and ref.ties == 0


def test_ref_from_tables_round_trips():
    ref = _ref(br.make_scene()[:3])
    again = lcr.ref_from_tables(ref.keyframe_table(), ref.landmark_table(), ref.observation_table(), dict(next_observation_id=ref.next_obs, next_landmark_id=ref.next_lm))
    for a, b in ((again.landmark_table(), ref.landmark_table()), (again.observation_table(), ref.observation_table()), (again.keyframe_table(), ref.keyframe_table())):
        assert all(a[k].tobytes() == b[k].tobytes() for k in b)
    kf = br.make_scene()[3]
    assert lc.add(again, kf) == lc.add(ref, kf) and again.landmark_table()["xyz"].tobytes() == ref.landmark_table()["xyz"].tobytes()
    assert all(again.window_table()[k].tobytes() == ref.window_table()[k].tobytes() for k in ref.window_table())
