"""Covisibility without a GPU (include/dvslam_hip.h "Covisibility"): the symbols declared and exported, the header as C99 with the struct
sizes the ctypes mirrors have, the argument errors that need no handle, the C++ adapter under plain g++, the restatement
(tests/covisibility_ref.py) against a brute-force double loop and a window worked out by hand on small tables, and the conditions the
scenes of tests/test_gpu_covisibility.py must meet, asserted on the restatement of the backend alone."""
import ctypes as C
import os
import re
import subprocess
import numpy as np
import pytest
import backend_ref as br
import covisibility_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "dynamic-visual-slam_amd", "lib")
NAMES = ["dvs_covis_default_params", "dvs_backend_covisibility", "dvs_backend_get_local_window", "dvs_backend_local_ba", "dvs_backend_track_frame_local"]


def test_symbols_declared_and_exported(hiplib, hooks):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dvslam_hip.h")).read(), flags=re.S)
    decl = set(re.findall(r"\b(dvs_[a-z0-9_]+)\s*\(", text))
    assert set(NAMES) <= decl and {n for n in decl if n.startswith("dvs_covis_")} == {"dvs_covis_default_params"}
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
                 'int main(void) { printf("%zu %zu %zu %zu %zu %d\\n", sizeof(dvs_covis_params), offsetof(dvs_covis_params, ba_max_iterations),\n'
                 '  sizeof(dvs_backend_lba_result), offsetof(dvs_backend_lba_result, n_cameras), offsetof(dvs_backend_lba_result, n_dropped),\n'
                 '  DVS_COVIS_MAX_KEYFRAMES); return 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), src, "-o", exe])
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [16, 12, 56, 32, 52, 8192]
    assert C.sizeof(B.CovisParams) == 16 and B.CovisParams.ba_max_iterations.offset == 12
    assert C.sizeof(B.LocalBaResult) == 56 and B.LocalBaResult.n_cameras.offset == 32 and B.LocalBaResult.n_dropped.offset == 52
    p = B.covis_params()
    assert {k: getattr(p, k) for k in cr.DEFAULTS} == cr.DEFAULTS
    with pytest.raises(TypeError):
        B.covis_params(min_wieght=3)


def test_null_arguments(hiplib):
    from dvslam_amd import backend as B, map_track as M
    B._bind(hiplib); M._bind(hiplib)
    n, m, r, t = C.c_int32(), C.c_int64(), B.LocalBaResult(), M.MapTrackResult()
    p = B.covis_params()
    none5 = [None] * 5
    assert hiplib.dvs_backend_covisibility(None, 15, 0, 0, None, None, None, None, C.byref(n), C.byref(m)) == -6
    assert hiplib.dvs_backend_get_local_window(None, 1, C.byref(p), 0, 0, 0, *none5, C.byref(n), *none5, C.byref(n), None, None, None, C.byref(n), None) == -6
    assert hiplib.dvs_backend_local_ba(None, None, 1, C.byref(p), C.byref(r)) == -6
    assert hiplib.dvs_backend_track_frame_local(None, None, 1, C.byref(p), None, None, 0, None, None, C.byref(t)) == -6
    assert b"bad argument" in hiplib.dvs_last_error()
    hiplib.dvs_covis_default_params(None)


def test_adapter_header_compiles_with_plain_gpp(hiplib, tmp_path):
    src = os.path.join(str(tmp_path), "adapter.cpp"); exe = os.path.join(str(tmp_path), "adapter")
    with open(src, "w") as fh:
        fh.write('#include <cstdio>\n#include "dvslam/covisibility.hpp"\n'
                 'int main() {\n  dvslam::CovisParams p;\n'
                 '  std::printf("%d %d %d %d %d\\n", p.min_weight, p.max_neighbours, p.max_fixed, p.ba_max_iterations, (int)sizeof(dvs_backend_lba_result));\n'
                 '  if (dvs_device_count() < 1) return 3;\n'
                 '  dvs_backend_params bp; dvs_backend_default_params(&bp); bp.fx = bp.fy = 500.0; bp.cx = 320.0; bp.cy = 240.0;\n'
                 '  dvslam::MappingBackend map(bp);\n  dvslam::CovisGraph g = dvslam::covisibilityGraph(map);\n'
                 '  try { dvslam::localWindow(map, 5); } catch (const std::runtime_error&) { return g.n == 0 && g.nb_offsets.size() == 1 ? 0 : 1; }\n'
                 '  return 1;\n}\n')
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), src, "-o", exe, "-L" + LIBDIR,
                           "-ldvslam_hip", "-Wl,-rpath," + LIBDIR, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode in (0, 3) and out.stdout.split() == ["15", "10", "32", "20", "56"], out.stdout[-2000:] + out.stderr[-2000:]


# ---------------------------------------------------------------------------------------------------- the restatement on hand-made tables
def _tables(frames, lm_ids, rows):
    """keyframes with those frame ids, landmarks with those ids, observation rows (frame id, landmark id) in table order"""
    nk, nl, no = len(frames), len(lm_ids), len(rows)
    kfs = dict(frame_id=np.array(frames, np.uint64), R=np.tile(np.eye(3), (nk, 1, 1)), t=np.arange(3.0 * nk).reshape(nk, 3))
    lms = dict(id=np.array(lm_ids, np.uint64), class_id=np.arange(nl, dtype=np.int32) % 3, xyz=np.arange(3 * nl, dtype=np.float32).reshape(nl, 3),
               desc=np.arange(32 * nl, dtype=np.int64).astype(np.uint8).reshape(nl, 32))
    obs = dict(frame_id=np.array([r[0] for r in rows], np.uint64), landmark_id=np.array([r[1] for r in rows], np.uint64),
               px=np.arange(2 * no, dtype=np.float32).reshape(no, 2), class_id=np.arange(no, dtype=np.int32) % 3)
    return kfs, lms, obs


# keyframe 10 names landmark 2 twice and the absent landmark 4; keyframe 13 has no rows; frame 99 is no keyframe; W[0][1] == W[0][2]
HAND = _tables([10, 11, 12, 13, 14], [1, 2, 3, 5, 8],
               [(10, 1), (10, 2), (10, 2), (10, 3), (10, 4), (11, 1), (11, 2), (11, 5), (12, 1), (12, 3), (12, 5), (12, 5), (12, 8), (14, 2), (14, 8), (99, 1)])
CHAIN = _tables([3, 1, 2], [7, 9], [(3, 7), (1, 7), (1, 9), (2, 9), (2, 9)])      # everybody is everybody's neighbour at theta = 1 but 3 - 2


def _brute_weights(kfs, lms, obs):
    n = len(kfs["frame_id"])
    rows = list(zip(obs["frame_id"].tolist(), obs["landmark_id"].tolist()))
    W = np.zeros((n, n), np.int32)
    for a in range(n):
        for b in range(n):
            for l in lms["id"].tolist():
                in_a = in_b = False
                for f, x in rows:
                    in_a = in_a or (f == kfs["frame_id"][a] and x == l)
                    in_b = in_b or (f == kfs["frame_id"][b] and x == l)
                W[a][b] += 1 if in_a and in_b else 0
    return W


@pytest.mark.parametrize("T", [HAND, CHAIN], ids=["hand", "chain"])
def test_graph_equals_a_brute_force_double_loop(T):
    W = _brute_weights(*T)
    n = len(W)
    for theta in (1, 2, 3):
        g = cr.graph(*T, theta)
        assert g["weights"].dtype == np.int32 and (g["weights"] == W).all() and (W == W.T).all()
        for a in range(n):
            want = []
            for w in range(int(W.max()), theta - 1, -1):                     # weight descending, then index ascending
                for b in range(n):
                    if b != a and W[a][b] == w:
                        want.append((b, w))
            lo, hi = g["nb_offsets"][a], g["nb_offsets"][a + 1]
            assert list(zip(g["nb_index"][lo:hi].tolist(), g["nb_weight"][lo:hi].tolist())) == want, (theta, a)
    with pytest.raises(ValueError):
        cr.graph(*T, 0)


def test_hand_table_has_every_case():
    W = cr.weights(cr.observes(*HAND))
    assert W.tolist() == [[3, 2, 2, 0, 1], [2, 3, 2, 0, 1], [2, 2, 4, 0, 1], [0, 0, 0, 0, 0], [1, 1, 1, 0, 2]]
    assert cr.repeated_pairs(*HAND) == 2
    assert cr.neighbours(W, 0, 2) == [(1, 2), (2, 2)] and cr.neighbours(W, 3, 1) == [] and cr.neighbours(W, 4, 1) == [(0, 1), (1, 1), (2, 1)]


def test_local_window_worked_out_by_hand():
    w = cr.local_window(*HAND, 10, min_weight=2, max_neighbours=1, max_fixed=1)
    assert w["kf_index"].tolist() == [0, 1, 2] and w["kf_frame_id"].tolist() == [10, 11, 12] and w["kf_fixed"].tolist() == [0, 0, 1]
    assert w["kf_weight"].tolist() == [3, 2, 2] and w["lm_id"].tolist() == [1, 2, 3, 5] and w["n_left_out"] == 2
    rows = [0, 1, 3, 5, 6, 7, 8, 9, 10]
    assert w["obs_landmark_id"].tolist() == [1, 2, 3, 1, 2, 5, 1, 3, 5] and w["obs_lm_index"].tolist() == [0, 1, 2, 0, 1, 3, 0, 2, 3]
    assert w["obs_px"].tobytes() == HAND[2]["px"][rows].tobytes() and w["obs_frame_id"].tolist() == [10] * 3 + [11] * 3 + [12] * 3
    assert w["lm_xyz"].tobytes() == HAND[1]["xyz"][[0, 1, 2, 3]].tobytes() and w["lm_class"].tolist() == [0, 1, 2, 0]
    # two fixed keyframes: 12 (three landmarks of U) before 14 (one); 13 observes nothing and never joins
    w = cr.local_window(*HAND, 10, min_weight=2, max_neighbours=1, max_fixed=5)
    assert w["kf_index"].tolist() == [0, 1, 2, 4] and w["kf_fixed"].tolist() == [0, 0, 1, 1] and w["kf_weight"].tolist() == [3, 2, 2, 1]
    # no neighbour passes: r alone is free, and the keyframes that see its landmarks are fixed in (f descending, index ascending)
    w = cr.local_window(*HAND, 10, min_weight=3, max_neighbours=10, max_fixed=2)
    assert w["kf_index"].tolist() == [0, 1, 2] and w["kf_fixed"].tolist() == [0, 1, 1] and w["lm_id"].tolist() == [1, 2, 3]
    # a keyframe without rows: alone, its own gauge, nothing to optimise
    w = cr.local_window(*HAND, 13, min_weight=1)
    assert w["kf_index"].tolist() == [3] and w["kf_fixed"].tolist() == [1] and len(w["lm_id"]) == 0 and len(w["obs_px"]) == 0 and w["n_left_out"] == 0
    xyz, desc, ids = cr.local_map(*HAND, 10, min_weight=2, max_neighbours=1)
    assert ids.tolist() == [1, 2, 3, 5] and ids.dtype == np.int64 and desc.tobytes() == HAND[1]["desc"][[0, 1, 2, 3]].tobytes()


def test_the_gauge_case_and_the_parameter_errors():
    w = cr.local_window(*CHAIN, 1, min_weight=1, max_neighbours=62, max_fixed=1)       # everything is free: the lowest index is the gauge
    assert w["kf_index"].tolist() == [0, 1, 2] and w["kf_fixed"].tolist() == [1, 0, 0] and w["kf_weight"].tolist() == [1, 2, 1] and w["n_left_out"] == 1
    w = cr.local_window(*CHAIN, 1, min_weight=1, max_neighbours=1, max_fixed=0)        # max_fixed = 0 leaves nobody fixed: the gauge again
    assert w["kf_index"].tolist() == [0, 1] and w["kf_fixed"].tolist() == [1, 0]
    for bad in (dict(min_weight=0), dict(max_neighbours=-1), dict(max_neighbours=63), dict(max_fixed=-1), dict(max_fixed=64),
                dict(max_neighbours=40, max_fixed=24), dict(ba_max_iterations=0)):
        with pytest.raises(ValueError):
            cr.local_window(*CHAIN, 1, **bad)
    with pytest.raises(ValueError):
        cr.local_window(*CHAIN, 4)
    cr.local_window(*CHAIN, 1, max_neighbours=40, max_fixed=23)


def test_local_ba_problem_drops_single_views(hiplib):
    w = cr.local_window(*HAND, 10, min_weight=2, max_neighbours=1, max_fixed=1)
    P, used, dropped = cr.local_ba_problem(w, 500.0, 500.0, 320.0, 240.0)
    assert used.tolist() == [True, True, True, True] and dropped == 0 and (P["K"], P["L"]) == (3, 4) and P["pose_fixed"].tolist() == [0, 0, 1]
    assert P["cam_idx"].tolist() == [0, 0, 0, 1, 1, 1, 2, 2, 2] and P["lm_idx"].tolist() == [0, 1, 2, 0, 1, 3, 0, 2, 3]
    w = cr.local_window(*HAND, 10, min_weight=3, max_neighbours=0, max_fixed=1)         # keyframes 10 and 11: landmark 3 is seen once
    P, used, dropped = cr.local_ba_problem(w, 500.0, 500.0, 320.0, 240.0)
    assert w["lm_id"].tolist() == [1, 2, 3] and used.tolist() == [True, True, False] and dropped == 1 and P["L"] == 2
    assert P["lm_idx"].tolist() == [0, 1, 0, 1] and P["uv"].tobytes() == HAND[2]["px"][[0, 1, 5, 6]].astype(np.float64).tobytes()


# ---------------------------------------------------------------------------------------------------- the scenes of the GPU tests
def test_hub_scene_meets_its_conditions():
    ref = cr.scene_ref(cr.hub_scene(), cls=cr.IncidenceRef)
    T = cr.tables(ref)
    assert ref.ties == 0 and len(T[1]["id"]) == 1 + cr.HUB_OWN + cr.HUB_BLOCK * len(cr.HUB_CLUSTERS)          # the association followed the incidence
    assert len(T[2]["id"]) == sum(len(s) for s in cr.hub_incidence())
    g1, g15 = cr.graph(*T, 1), cr.graph(*T, 15)
    cr.hub_conditions(g1, g15)
    S = cr.observes(*T)
    views = np.bincount(np.searchsorted(T[1]["id"], T[2]["landmark_id"]))
    assert views.max() == cr.HUB_NKF and len(S[cr.HUB]) == g1["weights"][cr.HUB][cr.HUB]
    # the windows the GPU test asks for: more neighbours than max_neighbours with equal weights, more fixed candidates than max_fixed
    w = cr.local_window(*T, cr.HUB_FRAME0 + cr.HUB, (S, g1["weights"]), max_neighbours=10, max_fixed=32)
    assert len(w["kf_index"]) == 43 and w["kf_fixed"].sum() == 32 and set(w["kf_weight"][w["kf_fixed"] == 0].tolist()) == {21, len(S[cr.HUB])}
    w = cr.local_window(*T, cr.HUB_FRAME0 + cr.HUB_LEAF, (S, g1["weights"]), max_neighbours=10, max_fixed=2)
    assert w["kf_index"].tolist().count(cr.HUB_LEAF) == 1 and (w["kf_fixed"] == 0).sum() == 1 and w["kf_fixed"].sum() == 2 and len(w["lm_id"]) == 4


def test_fused_scene_has_a_keyframe_that_names_a_landmark_twice():
    ref, out = cr.fused_ref()
    T = cr.tables(ref)
    assert out["n_fused"] > 0 and cr.repeated_pairs(*T) > 0
    kf_of = {int(f): k for k, f in enumerate(T[0]["frame_id"])}
    pairs = [(kf_of[int(f)], int(l)) for f, l in zip(T[2]["frame_id"], T[2]["landmark_id"])]
    assert max(pairs.count(p) for p in set(pairs)) >= 2
    SW = (cr.observes(*T), cr.weights(cr.observes(*T)))
    left = [cr.local_window(*T, f, SW, max_neighbours=m)["n_left_out"] for f in (100, 109) for m in (0, 3, 10)]
    assert max(left) > 0, left
    w = cr.local_window(*T, 109, SW)
    free = int((w["kf_fixed"] == 0).sum())
    P, used, dropped = cr.local_ba_problem(w, br.FX, br.FY, br.CX, br.CY)
    assert 2 <= free <= 16 and P["L"] > 50 and len(P["cam_idx"]) > 200 and len(set(zip(P["cam_idx"].tolist(), P["lm_idx"].tolist()))) == len(P["cam_idx"])


def test_maps_of_one_and_two_keyframes():
    scene = br.make_scene()
    for n in (1, 2):
        T = cr.tables(cr.scene_ref(scene[:n], filtered=(br.PERSON,)))
        g = cr.graph(*T, 1)
        assert g["weights"].shape == (n, n) and g["weights"][0][0] > 15
        w = cr.local_window(*T, 100)
        assert w["kf_fixed"].sum() == 1 and len(w["kf_index"]) == n
        if n == 2:
            assert g["weights"][0][1] > 15 and g["nb_index"].tolist() == [1, 0] and w["kf_fixed"].tolist() == [1, 0]
