"""Landmark refresh without a GPU (include/dvslam_hip.h "Landmark refresh"): the symbols declared and exported, the header as C99 with the
struct sizes the ctypes mirrors have, the argument errors that need no handle, the C++ adapter under plain g++, the restatement
(tests/landmark_refresh_ref.py) against a brute-force selection and cases worked out by hand, the FP64 geometry against a longdouble one
within the forward bound, and the conditions the scenes of tests/test_gpu_landmark_refresh.py must meet, asserted on the restatement alone."""
import ctypes as C
import os
import re
import subprocess
import numpy as np
import pytest
import landmark_refresh_ref as lr
import map_track_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "dynamic-visual-slam_amd", "lib")
NAMES = ["dvs_lm_refresh_default_params", "dvs_mapgate_default_gates", "dvs_backend_refresh_landmarks", "dvs_backend_get_landmark_geometry",
         "dvs_mapgate_search_device", "dvs_mapgate_track_device", "dvs_mapgate_get_counts", "dvs_backend_track_frame_gated",
         "dvs_tracker_track_map_gated"]


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


def test_header_is_c99_and_the_structs_match_their_mirrors(hiplib, tmp_path):
    from dvslam_amd import backend as B
    src = os.path.join(str(tmp_path), "sizes.c"); exe = os.path.join(str(tmp_path), "sizes")
    with open(src, "w") as fh:
        fh.write('#include <stdio.h>\n#include <stddef.h>\n#include "dvslam_hip.h"\n'
                 'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(dvs_lm_refresh_params), offsetof(dvs_lm_refresh_params, use_scope),\n'
                 '  offsetof(dvs_lm_refresh_params, scope_frame_id), sizeof(dvs_lm_refresh_result), offsetof(dvs_lm_refresh_result, max_views),\n'
                 '  sizeof(dvs_maptrack_gates), offsetof(dvs_maptrack_gates, range_factor), sizeof(dvs_maptrack_result));\n  return 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), src, "-o", exe])
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [24, 8, 16, 16, 12, 16, 8, 128]
    assert C.sizeof(B.LmRefreshParams) == 24 and B.LmRefreshParams.use_scope.offset == 8 and B.LmRefreshParams.scope_frame_id.offset == 16
    assert C.sizeof(B.LmRefreshResult) == 16 and B.LmRefreshResult.max_views.offset == 12
    assert C.sizeof(B.MapTrackGates) == 16 and B.MapTrackGates.range_factor.offset == 8
    p = B.lm_refresh_params()
    assert (p.update_descriptors, p.min_views, p.use_scope, p.reserved, p.scope_frame_id) == (1, 1, 0, 0, 0)
    q = B.lm_refresh_params(77, min_views=3, update_descriptors=0)
    assert (q.update_descriptors, q.min_views, q.use_scope, q.scope_frame_id) == (0, 3, 1, 77)
    g = B.maptrack_gates()
    assert {k: getattr(g, k) for k in lr.DEFAULT_GATES} == lr.DEFAULT_GATES
    with pytest.raises(TypeError):
        B.lm_refresh_params(min_view=3)
    with pytest.raises(TypeError):
        B.maptrack_gates(cos=0.5)


def test_null_and_argument_errors_come_before_any_handle_work(hiplib):
    from dvslam_amd import backend as B, map_track as M
    B._bind(hiplib); M._bind(hiplib)
    n, r, res = C.c_int32(), B.LmRefreshResult(), M.MapTrackResult()
    p = B.lm_refresh_params()
    assert hiplib.dvs_backend_refresh_landmarks(None, C.byref(p), C.byref(r)) == -6
    assert b"bad argument" in hiplib.dvs_last_error()
    hiplib.dvs_lm_refresh_default_params(None); hiplib.dvs_mapgate_default_gates(None)
    assert hiplib.dvs_backend_get_landmark_geometry(None, 0, None, None, None, None, None, C.byref(n)) == -6
    assert hiplib.dvs_mapgate_get_counts(None, None) == -6
    assert hiplib.dvs_backend_track_frame_gated(None, None, None, None, None, 0, None, None, C.byref(res)) == -6
    assert hiplib.dvs_tracker_track_map_gated(None, None, None, None, 0, C.byref(res)) == -6
    # the parameters are judged before the handle is read: any non-null address does for one
    fake = C.create_string_buffer(64)
    h = C.cast(fake, C.c_void_p)
    assert hiplib.dvs_backend_refresh_landmarks(h, C.byref(B.lm_refresh_params(min_views=0)), C.byref(r)) == -6
    assert hiplib.dvs_backend_get_landmark_geometry(h, 0, None, None, None, None, None, None) == -6          # no n
    assert hiplib.dvs_backend_get_landmark_geometry(h, -1, None, None, None, None, None, C.byref(n)) == -6   # cap < 0
    assert hiplib.dvs_mapgate_get_counts(h, None) == -6
    R, t = np.eye(3).reshape(9), np.zeros(3)
    for fn in (hiplib.dvs_mapgate_search_device, hiplib.dvs_mapgate_track_device):
        for bad in (dict(cos_min=-0.01), dict(cos_min=1.01), dict(cos_min=float("nan")), dict(range_factor=0.99), dict(range_factor=float("inf")),
                    dict(range_factor=float("nan"))):
            g = B.maptrack_gates(**bad)
            assert fn(h, None, None, None, 0, None, None, None, C.byref(g), None, None, 0, R.ctypes.data, t.ctypes.data, C.byref(res)) == -6, bad
            assert b"bad argument" in hiplib.dvs_last_error()
        g = B.maptrack_gates()
        assert fn(h, None, None, None, 3, None, None, None, C.byref(g), None, None, 0, R.ctypes.data, t.ctypes.data, C.byref(res)) == -6   # rows announced, none given
        assert fn(None, None, None, None, 0, None, None, None, C.byref(g), None, None, 0, R.ctypes.data, t.ctypes.data, C.byref(res)) == -6
    assert fake.raw == bytes(64)


def test_adapter_header_compiles_with_plain_gpp(hiplib, tmp_path):
    src = os.path.join(str(tmp_path), "adapter.cpp"); exe = os.path.join(str(tmp_path), "adapter")
    with open(src, "w") as fh:
        fh.write('#include <cstdio>\n#include "dvslam/landmark_refresh.hpp"\n'
                 'int main() {\n  dvslam::LandmarkRefreshParams p; dvslam::MapTrackGates g;\n'
                 '  std::printf("%d %d %d %.2f %.2f %d\\n", p.update_descriptors, p.min_views, p.use_scope, g.cos_min, g.range_factor, (int)sizeof(dvs_lm_refresh_result));\n'
                 '  if (dvs_device_count() < 1) return 3;\n'
                 '  dvs_backend_params bp; dvs_backend_default_params(&bp); bp.fx = bp.fy = 500.0; bp.cx = 320.0; bp.cy = 240.0;\n'
                 '  dvslam::MappingBackend map(bp);\n  dvs_lm_refresh_result r = dvslam::refreshLandmarks(map, p);\n'
                 '  dvslam::LandmarkGeometry geo = dvslam::landmarkGeometry(map);\n'
                 '  if (r.n_in_scope != 0 || r.n_changed != 0 || !geo.normal.empty() || !geo.best_obs_id.empty()) return 1;\n'
                 '  dvslam::MapTracker mt(dvslam::MapTracker::defaultParams(480, 640, 500.0, 500.0, 320.0, 240.0));\n'
                 '  const double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {0, 0, 0};\n  std::array<int32_t, 4> counts{{9, 9, 9, 9}};\n'
                 '  dvs_maptrack_result tr = dvslam::trackFrameGated(map, mt, nullptr, nullptr, 0, R, t, g, &counts);\n'
                 '  if (tr.status != DVS_MAPTRACK_FEW_MATCHES || counts[0] || counts[1] || counts[2] || counts[3]) return 1;\n'
                 '  try { dvslam::refreshLandmarks(map, 5, p); } catch (const std::runtime_error&) { return 0; }\n'
                 '  return 1;\n}\n')
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), src, "-o", exe, "-L" + LIBDIR,
                           "-ldvslam_hip", "-Wl,-rpath," + LIBDIR, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode in (0, 3) and out.stdout.split() == ["1", "1", "0", "0.50", "2.00", "16"], out.stdout[-2000:] + out.stderr[-2000:]


# ---------------------------------------------------------------------------------------------------- the selection
def _brute(desc):
    """numpy.sort per row, the candidates ordered by a stable argsort"""
    D = lr.distances(desc)
    med = np.sort(D, axis=1)[:, (len(D) - 1) // 2]
    i = int(np.argsort(med, kind="stable")[0])
    return i, int(med[i])


def _word(*bits):
    return lr.flip(np.zeros(32, np.uint8), bits)


def test_selection_by_hand():
    """n = 2: D = [[0, d], [d, 0]], index 0 of each sorted row is 0, so both medians are 0 and the first view is chosen.
    n = 4 with descriptors a = 0, b = bits {0, 1}, c = bits {0, 1, 2, 3}, d = bits {0 .. 5}: the rows sorted are a: 0 2 4 6, b: 0 2 2 4, c: 0 2 2 4,
    d: 0 2 4 6, the element at index 1 is 2 for every row: a four-way tie, the first view wins.  With a replaced by bits {10 .. 19} (ten bits
    the others do not have) its row is 0 12 14 16 and b, c, d keep 2: b, the first of the tie, is chosen."""
    assert lr.select([_word(), _word(*range(40))]) == (0, 0)
    assert lr.select([_word(*range(40)), _word()]) == (0, 0)
    four = [_word(), _word(0, 1), _word(0, 1, 2, 3), _word(0, 1, 2, 3, 4, 5)]
    assert lr.distances(four).tolist() == [[0, 2, 4, 6], [2, 0, 2, 4], [4, 2, 0, 2], [6, 4, 2, 0]]
    assert lr.select(four) == (0, 2)
    four[0] = _word(*range(10, 20))
    assert lr.distances(four)[0].tolist() == [0, 12, 14, 16] and lr.select(four) == (1, 2)
    assert lr.select([_word(3)]) == (0, 0)
    three = [_word(*range(9)), _word(), _word(0)]                          # rows sorted: 0 8 9, 0 1 9, 0 1 8 -> medians 8, 1, 1
    assert lr.select(three) == (1, 1)


def test_selection_equals_the_brute_force_version():
    rng = np.random.default_rng(3)
    for n in (1, 2, 3, 4, 5, 8, 9, 17, 64, 65, 130):
        for spread in (0, 1, 3, 30):                                       # 0: identical descriptors; small: many equal medians
            base = rng.integers(0, 256, 32, dtype=np.uint8)
            desc = [lr.flip(base, rng.choice(256, int(rng.integers(0, spread + 1)), replace=False)) for _ in range(n)]
            assert lr.select(desc) == _brute(desc), (n, spread)


def _hand_tables():
    """keyframes 10, 11, 12 at (0,0,0), (3,0,0), (0,0,0); frame 99 is no keyframe.  Landmark 1 at (0,0,4) is seen by 10 (r = 4), by 11
    (d = (-3, 0, 4), r = 5), by frame 99 (does not count); landmark 2 at (0,0,0) by 10 and 12, both at its own position (r = 0: no view counts);
    landmark 3 has no row.  Keyframe 10 names landmark 1 twice."""
    kfs = dict(frame_id=np.array([10, 11, 12], np.uint64), t=np.array([[0, 0, 0], [3, 0, 0], [0, 0, 0]], np.float64))
    lms = dict(id=np.array([1, 2, 3], np.uint64), xyz=np.array([[0, 0, 4], [0, 0, 0], [1, 1, 1]], np.float32), desc=np.zeros((3, 32), np.uint8))
    rows = [(10, 1), (11, 1), (10, 2), (99, 1), (12, 2), (10, 1)]
    obs = dict(id=np.arange(100, 106, dtype=np.uint64), frame_id=np.array([r[0] for r in rows], np.uint64), landmark_id=np.array([r[1] for r in rows], np.uint64),
               desc=np.array([_word(0), _word(0, 1), _word(), _word(0, 1, 2), _word(7), _word(0)], np.uint8))
    return kfs, lms, obs


def test_geometry_and_refresh_by_hand():
    kfs, lms, obs = _hand_tables()
    g = lr.geometry(kfs, lms, obs)
    assert g["n_counted"].tolist() == [3, 0, 0]
    assert g["range"].tolist() == [[4.0, 5.0], [0.0, 0.0], [0.0, 0.0]]
    # the views of landmark 1 that count, in view order: 10 (0, 0, 1), 11 (-0.6, 0, 0.8), 10 again (0, 0, 1)
    assert g["normal"][0].tolist() == [(0.0 + -3.0 / 5.0 + 0.0) / 3.0, 0.0, ((1.0 + 4.0 / 5.0) + 1.0) / 3.0] and not g["normal"][1:].any()
    # landmark 1's views: rows 0, 1, 3, 5 with bits {0}, {0, 1}, {0, 1, 2}, {0}: rows sorted 0 0 1 2 | 0 1 1 1 | 0 1 2 2 | 0 0 1 2 -> medians 0, 1, 1, 0
    assert g["best_obs_id"].tolist() == [100, 102, int(lr.NO_VIEW_ID)] and g["best_median"].tolist() == [0, 0, -1]
    res, desc = lr.refresh(kfs, lms, obs)
    assert res == dict(n_in_scope=3, n_changed=1, n_without_views=1, max_views=4)
    assert desc[0].tobytes() == _word(0).tobytes() and not desc[1:].any()
    res, desc = lr.refresh(kfs, lms, obs, min_views=3)
    assert res["n_changed"] == 1
    res, desc = lr.refresh(kfs, lms, obs, min_views=5)
    assert res["n_changed"] == 0 and not desc.any()
    res, _ = lr.refresh(kfs, lms, obs, scope_frame_id=12)
    assert res == dict(n_in_scope=1, n_changed=0, n_without_views=0, max_views=2)
    res, _ = lr.refresh(kfs, lms, obs, scope_frame_id=11, update_descriptors=0)
    assert res == dict(n_in_scope=1, n_changed=1, n_without_views=0, max_views=4)
    with pytest.raises(ValueError):
        lr.refresh(kfs, lms, obs, scope_frame_id=99)


def _random_tables(seed, nkf=40, nlm=30):
    rng = np.random.default_rng(seed)
    kfs = dict(frame_id=np.arange(50, 50 + nkf, dtype=np.uint64), t=rng.uniform(-2, 2, (nkf, 3)))
    lms = dict(id=np.arange(nlm, dtype=np.uint64), xyz=rng.uniform(-3, 3, (nlm, 3)).astype(np.float32), desc=np.zeros((nlm, 32), np.uint8))
    rows = [(50 + int(rng.integers(0, nkf)), int(rng.integers(0, nlm))) for _ in range(20 * nlm)] + [(50 + k, 0) for k in range(nkf)] * 8
    obs = dict(id=np.arange(len(rows), dtype=np.uint64), frame_id=np.array([r[0] for r in rows], np.uint64), landmark_id=np.array([r[1] for r in rows], np.uint64),
               desc=rng.integers(0, 256, (len(rows), 32), dtype=np.uint8))
    return kfs, lms, obs


def test_fp64_geometry_lies_within_the_forward_bound_of_longdouble():
    """a forward bound, not a measurement: each d / r carries the subtraction's, the square root's and the division's roundings (sqrt and
    division within 2 ulp assumed), and a sum of m terms of magnitude <= 1 adds m more: (m + 32) * 2^-53 absolute per component; dmin and
    dmax are one such r: 16 * 2^-53 relative"""
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63, "numpy.longdouble must be wider than double for this comparison"
    for seed in (1, 2):
        T = _random_tables(seed)
        a, b = lr.geometry(*T), lr.geometry(*T, real=np.longdouble)
        assert (a["n_counted"] == b["n_counted"]).all() and a["n_counted"].max() >= 320
        for s, m in enumerate(a["n_counted"]):
            assert np.abs(a["normal"][s] - b["normal"][s]).max() <= lr.NORMAL_BOUND(int(m)), (s, m)
            assert (np.abs(a["range"][s] - b["range"][s]) <= lr.RANGE_BOUND * np.abs(b["range"][s])).all(), s


# ---------------------------------------------------------------------------------------------------- the gates
def test_gates_by_hand_at_exact_equality():
    """O = 0, X = (0, 0, 2): q = 4.  dmin = 4 with range_factor 2 gives a * a = 4: q < 4 is false.  dmax = 1 gives b * b = 4: q > 4 is false.
    N = (0, 0, 0.5): s = 1, s * s = 1, cc * q = 0.25 * 4 = 1: 1 < 1 is false.  Every number is a small dyadic rational, so each is exact."""
    X, O = [0.0, 0.0, 2.0], [0.0, 0.0, 0.0]
    for args, want in lr.EXACT_GATE_CASES:
        assert lr.gate(X, O, *args)[0] == want, args


def test_the_gate_scene_meets_its_conditions():
    P = mr.frame_params()
    for n_lm in (63, 64, 65, 255, 256, 257):
        xyz, _, _, _, normal, rg, cnt, R, t = lr.gate_scene(P, n_lm, 120, 100 + n_lm)
        g, counts = lr.gates(xyz, t, normal, rg, cnt)
        assert g.tolist() == [(-1, 0, 1, 2, 3, -1)[j % 6] for j in range(n_lm)]
        assert counts.sum() == sum(1 for j in range(n_lm) if j % 6 in (1, 2, 3, 4)) and (counts >= 10).all()
        assert lr.gate_margin(xyz, t, normal, rg, cnt) > 1e-9
        gl, _ = lr.gates(xyz, t, normal, rg, cnt, real=np.longdouble)
        assert (gl == g).all()


# ---------------------------------------------------------------------------------------------------- the scenes
def test_the_views_scene_is_what_the_gpu_tests_need():
    kfs, counts = lr.views_scene()
    assert len(kfs) == 301 and counts[:len(lr.VIEW_COUNTS)] == lr.VIEW_COUNTS
    small = sum(1 for c in counts if c <= 8); wave = sum(1 for c in counts if 8 < c <= 64)
    assert small > 8 and wave > 4 and sum(1 for c in counts if c > 64) == 5            # more than a wavefront takes, more than a workgroup takes; five workgroups
    seen = {}
    for kf in kfs[:300]:
        for x, d in zip(kf["xyz"], kf["desc"]):
            seen.setdefault(x.tobytes(), []).append(d)
    assert sorted(len(v) for v in seen.values()) == sorted(counts)
    ties = 0
    for v in seen.values():
        assert max(mr.hamming(v[0], d) for d in v) <= 40 < 49                            # every view associates with the first view's landmark
        if len(v) >= 3:
            D = lr.distances(v)
            med = np.sort(D, axis=1)[:, (len(v) - 1) // 2]
            ties += (med == med.min()).sum() > 1
    assert ties >= 10                                                                    # rows with equal smallest medians: the index decides


def test_the_drift_scene_counts_are_as_designed():
    """view 1 is chosen for every drifting point; with the first view's descriptor the query matches no drifting point, with the chosen one all"""
    kfs, q = lr.drift_scene()
    P = lr.track_params()
    n = lr.DRIFT_N + lr.DRIFT_STATIC
    views = [[] for _ in range(n)]
    X = np.zeros((n, 3)); rows = {}
    for kf in kfs:
        for x, d in zip(kf["xyz"], kf["desc"]):
            j = rows.setdefault(x.tobytes(), len(rows))
            X[j] = x; views[j].append(d)
    assert len(rows) == n and all(len(v) == lr.DRIFT_NKF for v in views)
    xyz = X.astype(np.float32)
    drifting = np.array([mr.hamming(v[0], v[-1]) == lr.DRIFT_STEP * (lr.DRIFT_NKF - 1) for v in views])
    assert drifting.sum() == lr.DRIFT_N
    for v, dr in zip(views, drifting):
        if dr:
            assert lr.distances(v)[0].tolist() == [lr.DRIFT_STEP * k for k in range(lr.DRIFT_NKF)] and lr.select(v) == (1, 12)
    before = dict(xyz=xyz, desc=np.array([v[0] for v in views], np.uint8))
    after = np.array([v[lr.select(v)[0]] for v in views], np.uint8)
    # which keypoint shows which point: the nearest descriptor (54 bits at most; two points are about 128 apart)
    kp_of = np.array([int(np.argmin([mr.hamming(before["desc"][j], kd) for kd in q["kdesc"]])) for j in range(n)])
    assert sorted(kp_of.tolist()) == list(range(n))
    kd = np.array([mr.hamming(before["desc"][j], q["kdesc"][kp_of[j]]) for j in range(n)])
    assert sorted(set(kd[drifting].tolist())) == [lr.DRIFT_QUERY_BITS] and not kd[~drifting].any()
    m0 = lr.matched_keypoints(P, q["R"], q["t"], before, q["kps"], q["kdesc"])
    m1 = lr.matched_keypoints(P, q["R"], q["t"], before, q["kps"], q["kdesc"], after)
    assert not m0[q["drifting"]].any() and m0[~q["drifting"]].all() and m1.all()
    assert m0.sum() == lr.DRIFT_STATIC >= P.min_matches


def test_the_wall_scene_proposes_back_side_landmarks_without_the_gate():
    kfs, q = lr.wall_scene()
    P = lr.track_params()
    F, B = kfs[0]["xyz"], kfs[3]["xyz"]
    xyz = np.concatenate([F, B]).astype(np.float32); desc = np.concatenate([kfs[0]["desc"], kfs[3]["desc"]])
    Rcw, tcw = mr.pose_cw(q["R"], q["t"])
    rec = mr.search_grid(P, Rcw, tcw, xyz, desc, q["kps"], q["kdesc"])
    assert rec["proposed"].all() and (rec["d_best"][:lr.WALL_N] == 0).all() and (rec["d_best"][lr.WALL_N:] == 30).all() and (rec["d_second"] == -1).all()
    # the geometry the map will hold: front landmarks seen from z = 0, back landmarks from z = 8
    kf_t = np.array([k["t"] for k in kfs])
    normal = np.zeros((2 * lr.WALL_N, 3)); rg = np.zeros((2 * lr.WALL_N, 2))
    for j in range(2 * lr.WALL_N):
        d = xyz[j].astype(np.float64) - (kf_t[:3] if j < lr.WALL_N else kf_t[3:])
        r = np.linalg.norm(d, axis=1)
        normal[j] = (d / r[:, None]).mean(0); rg[j] = (r.min(), r.max())
    g, counts = lr.gates(xyz, q["t"], normal, rg, np.full(2 * lr.WALL_N, 3))
    assert (g[:lr.WALL_N] == -1).all() and (g[lr.WALL_N:] == lr.BACK).all() and counts.tolist() == [0, 0, lr.WALL_N, 0]
    assert lr.gate_margin(xyz, q["t"], normal, rg, np.full(2 * lr.WALL_N, 3)) > 1e-3
