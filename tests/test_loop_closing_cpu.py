"""Loop closing on the map without a GPU (include/dvslam_hip.h "Loop closing on the map"): the new symbols declared and exported, the header
as C99, the new structs against their ctypes mirrors, argument errors without a handle, the C++ adapter under plain g++, the fusion rule
checked by hand on a map written out below, and the fixture conditions of the scene the GPU tests use (tests/loop_closing_ref.py), asserted
on the restatement alone so that no GPU test can pass vacuously."""
import ctypes as C
import os
import re
import subprocess
import numpy as np

import backend_ref as br
from compaction_scenes import crosses_blocks
import loop_closing_ref as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["dvs_fuse_default_params", "dvs_backend_get_anchors", "dvs_backend_build_pose_graph", "dvs_backend_close_loop", "dvs_backend_fuse"]


def test_symbols_declared_and_exported(hiplib):
    from dvslam_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dvslam_hip.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.SO_PATH], capture_output=True, text=True, check=True).stdout
    product = set(line.split()[-1] for line in out.splitlines() if line.strip())
    for s in SYMBOLS:
        assert re.search(r"\b" + s + r"\s*\(", header), s
        assert s in product, s
    assert sorted(n for n in product if n.startswith("dvs_fuse_")) == ["dvs_fuse_default_params"]
    full = open(os.path.join(ROOT, "include", "dvslam_hip.h")).read()
    assert "Loop closing on the map" in full and "SearchAndFuse" in full and "CorrectLoop" in full


def test_header_compiles_as_c_and_structs_match_the_mirror(tmp_path):
    from dvslam_amd import backend as B
    src = tmp_path / "sizes.c"
    src.write_text('#include "dvslam_hip.h"\n#include <stdio.h>\nint main(void) { dvs_fuse_params p; dvs_close_loop_result r; r.fuse.n_fused = 0; p.fuse_neighbours = 0; '
                   'printf("%zu %zu %zu\\n", sizeof(dvs_fuse_params), sizeof(dvs_fuse_result), sizeof(dvs_close_loop_result)); '
                   'return r.fuse.n_fused + p.fuse_neighbours; }\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    sizes = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert sizes == [C.sizeof(B.FuseParams), C.sizeof(B.FuseResult), C.sizeof(B.CloseLoopResult)] == [24, 16, 64]


def test_adapter_header_compiles(tmp_path):
    src = tmp_path / "use.cpp"
    src.write_text('#include "dvslam/loop_closing.hpp"\n'
                   'int main() { dvslam::FuseParams f; dvslam::LoopEdge e; e.w_rot = 1; return f.fuse_neighbours == 2 && sizeof(&dvslam::closeLoop) > 0 ? 0 : 1; }\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)


def test_null_handles_and_defaults(hiplib):
    from dvslam_amd import backend as B
    L = B._bind(hiplib)
    p = B.FuseParams()
    assert L.dvs_fuse_default_params(None) == -6 and L.dvs_fuse_default_params(C.byref(p)) == 0
    assert (p.max_descriptor_distance, p.max_reprojection_distance, p.fuse_neighbours) == (50.0, 5.0, 2) == tuple(lc.FUSE_DEFAULTS[k] for k in (
        "max_descriptor_distance", "max_reprojection_distance", "fuse_neighbours"))
    n, m = C.c_int32(), C.c_int32()
    r, cr = B.FuseResult(), B.CloseLoopResult()
    ids = np.zeros(1, np.uint64)
    assert L.dvs_backend_get_anchors(None, 0, None, None, C.byref(n)) == -6
    assert L.dvs_backend_build_pose_graph(None, 0, None, None, None, None, None, None, 1.0, 1.0, 0, 0, None, None, None, None, None, None, None, None, None,
                                          C.byref(n), C.byref(m)) == -6
    assert L.dvs_backend_close_loop(None, None, 0, None, None, None, None, None, None, 1.0, 1.0, None, None, C.byref(cr)) == -6
    assert L.dvs_backend_fuse(None, 0, ids.ctypes.data, 1, None, 0, C.byref(r), 0, None, None, None, C.byref(n)) == -6


# ---- the rule by hand ---------------------------------------------------------------------------------------------------------------
# Camera: backend_ref.Q_Z180 (R = diag(-1, -1, 1)) at the origin, f = 600, c = (320, 240): X = (x, y, z) projects to (320 - 600 x / z, 240 - 600 y / z).
#   keyframe 0 (frame 1, the entry) holds four observations, one of each SOURCE:
#     S0 id 0  (-1.5, -0.75,  3) -> (620, 390) exactly      descriptor d0
#     S1 id 1  the same position and descriptor as S0: an exact tie in e
#     S2 id 2  ( 0,    0,     3) -> (320, 240)              descriptor d2
#     S3 id 3  ( 0,    0,    -3)  behind the camera         descriptor d3
#   keyframe 1 (frame 2, the query) holds three observations, each naming its own TARGET (ids 10, 11, 12; their positions play no part):
#     o0 id 4  pixel (621, 390)  class 0  descriptor d0     e(S0) = e(S1) = 1: both propose, the lower id S0 wins
#     o1 id 5  pixel (320, 240)  class 1  descriptor d2     e(S2) = 0, but S2 is class 0: no candidate
#     o2 id 6  pixel (1, 1.5)    class 0  descriptor d3     reprojection_error's (-1, -1) stand-in would give e = 3.2 < 5: must not fuse
def _hand_map():
    rng = np.random.default_rng(0)
    d = rng.integers(0, 256, (4, 32), dtype=np.uint8)
    ref = br.BackendRef(600.0, 600.0, 320.0, 240.0)
    R = br.quat_to_R(br.Q_Z180); t = np.zeros(3)
    ref.kfs = [dict(frame=1, R=R.copy(), t=t.copy(), stamp=10**9, obs_ids=[0, 1, 2, 3]), dict(frame=2, R=R.copy(), t=t.copy(), stamp=2 * 10**9, obs_ids=[4, 5, 6])]
    pos = [(-1.5, -0.75, 3.0), (-1.5, -0.75, 3.0), (0.0, 0.0, 3.0), (0.0, 0.0, -3.0)]
    desc = [d[0], d[0], d[2], d[3]]
    ref.db = {0: {}, 1: {}}
    for k in range(4):
        ref.db[0][k] = dict(id=k, cls=0, pos=np.array(pos[k], np.float32), desc=desc[k].copy(), obs_ids=[k], count=1 + k, last_seen=10**9)
        ref.obs.append(dict(id=k, frame=1, px=np.array([50.0 + k, 60.0], np.float32), desc=desc[k].copy(), cls=0, lm=k))
    q = [((621.0, 390.0), 0, d[0]), ((320.0, 240.0), 1, d[2]), ((1.0, 1.5), 0, d[3])]
    for k, (px, cls, dd) in enumerate(q):
        ref.db[cls][10 + k] = dict(id=10 + k, cls=cls, pos=np.array((9.0, 9.0, 9.0), np.float32), desc=dd.copy(), obs_ids=[4 + k], count=7, last_seen=2 * 10**9)
        ref.obs.append(dict(id=4 + k, frame=2, px=np.array(px, np.float32), desc=dd.copy(), cls=cls, lm=10 + k))
    ref.next_obs, ref.next_lm = 7, 13
    return ref


def test_fusion_rule_by_hand():
    ref = _hand_map()
    kq = ref.kfs[1]
    # the stand-in that must not fuse: the plain reprojection error of the point behind the camera IS below the gate
    assert br.reprojection_error(ref.obs[6]["px"], ref.db[0][3]["pos"], kq["R"], kq["t"], *ref.K) < 5.0
    assert br.reprojection_error(ref.obs[5]["px"], ref.db[0][2]["pos"], kq["R"], kq["t"], *ref.K) == 0.0
    before = (ref.landmark_table(), ref.observation_table())
    dry = lc.fuse(ref, 2, [1], apply=False)
    assert dry == dict(n_sources=4, n_targets=3, n_proposals=2, n_fused=1, pairs=[(0, 10, 1.0)])
    after = (ref.landmark_table(), ref.observation_table())
    assert all(before[k][c].tobytes() == after[k][c].tobytes() for k in range(2) for c in before[k]), "a dry run must not modify the map"
    assert lc.fuse(ref, 2, [1], apply=True) == dry
    L, O = ref.landmark_table(), ref.observation_table()
    assert L["id"].tolist() == [0, 1, 2, 3, 11, 12]
    assert L["observation_count"].tolist() == [1 + 7, 2, 3, 4, 7, 7] and L["last_seen_ns"][0] == 2 * 10**9
    assert L["xyz"][0].tolist() == [-1.5, -0.75, 3.0]
    assert O["landmark_id"].tolist() == [0, 1, 2, 3, 0, 11, 12] and O["id"].tolist() == list(range(7))
    assert L["obs_ids"][L["obs_offsets"][0]:L["obs_offsets"][1]].tolist() == [0, 4]
    assert (ref.next_obs, ref.next_lm) == (7, 13) and ref.kfs[1]["obs_ids"] == [4, 5, 6]
    ids, anc = lc.anchors(ref)
    assert ids.tolist() == [0, 1, 2, 3, 11, 12] and anc.tolist() == [0, 0, 0, 0, 1, 1]
    # an observation whose landmark left the table is nobody's target, and a landmark without observations has no anchor
    lost = _hand_map()
    del lost.db[0][10]
    lost.obs = [o for o in lost.obs if o["id"] != 3]
    assert lc.fuse(lost, 2, [1], apply=True) == dict(n_sources=3, n_targets=2, n_proposals=0, n_fused=0, pairs=[])
    assert lc.anchors(lost)[1].tolist() == [0, 0, 0, -1, 1, 1]
    # a second fusion sees the merge of the first: o0 now names S0, which makes S0 a target, and its twin S1 still reprojects on o0
    again = lc.fuse(ref, 2, [1], apply=True)
    assert again["n_fused"] == 1 and again["pairs"] == [(0, 1, 1.0)], "the tied twin S1 now merges into S0 itself"


def test_pose_graph_of_the_hand_map():
    ref = _hand_map()
    ref.kfs[1]["t"] = np.array([0.5, -0.25, 0.0])
    g = lc.build_pose_graph(ref, [(2, 1, (0.0, 0.0, 0.1), (0.1, 0.2, 0.3), 3.0, 4.0)], (10.0, 20.0))
    assert g["fixed"].tolist() == [1, 0] and g["ei"].tolist() == [0, 1] and g["ej"].tolist() == [1, 0]
    assert g["w_rot"].tolist() == [10.0, 3.0] and g["w_trans"].tolist() == [20.0, 4.0]
    assert g["rvec"][0].tolist() == [0.0, 0.0, 0.0] and g["tvec"][0].tolist() == [-0.5, 0.25, 0.0]      # R_a^T (t_b - t_a) with R = diag(-1, -1, 1)
    assert g["rvec"][1].tolist() == [0.0, 0.0, 0.1] and g["tvec"][1].tolist() == [0.1, 0.2, 0.3]


def test_scene_fixture_conditions():
    scene, truth = lc.scene()
    ref, results = lc.scene_ref()
    assert len(scene) == lc.NKF and all(250 <= len(kf["px"]) <= 350 for kf in scene)
    assert ref.ties == 0
    drift = np.linalg.norm(scene[-1]["t"] - truth["t"][-1])
    assert 0.19 < drift < 0.21
    # the world point behind every landmark: the point of its first observation
    point_of_obs = {}
    oid = 0
    for pts in truth["point"]:
        for p in pts:
            point_of_obs[oid] = int(p); oid += 1
    assert oid == ref.next_obs, "no class is filtered: observation ids follow the message order"
    lm_point = {}
    for o in ref.obs:
        lm_point.setdefault(o["lm"], point_of_obs[o["id"]])
    first = {}
    for lid in sorted(lm_point):
        first.setdefault(lm_point[lid], lid)
    last = results[-1]
    assert last["n_associated"] == 0, "the drift must keep the last keyframe from associating with the old landmarks"
    duplicates = [lid for lid in lm_point if lid >= last["first_landmark_id"] and first[lm_point[lid]] != lid]
    assert len(duplicates) >= 150, len(duplicates)
    ids_before = ref.landmark_table()["id"]
    out = lc.close_loop(ref, lc.scene_loop(), lc.ODO_W, fuse_params={})
    assert out["termination"] == 0 and out["n_landmarks_moved"] == len(lm_point)
    assert crosses_blocks(ids_before, ref.landmark_table()["id"]) == (True, True), "fusion's compaction must work across workgroups"
    (pairs,) = out["pairs"]
    assert out["n_fused"] == len(pairs) >= 100, out["n_fused"]
    assert out["n_proposals"] > out["n_fused"], "some targets must choose among several proposals"
    assert all(lm_point[s] == lm_point[g] for s, g, _ in pairs), "every merged pair must be a true duplicate"
    assert all(s < g for s, g, _ in pairs) and [g for _, g, _ in pairs] == sorted(g for _, g, _ in pairs)
    assert ref.ties == 0
