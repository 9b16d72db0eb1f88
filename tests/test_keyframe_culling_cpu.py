"""Keyframe culling without a GPU (include/dvslam_hip.h "Keyframe culling"): the symbols declared and exported, the header as C99 with the
struct sizes the ctypes mirrors have, the argument errors that need no handle, the C++ adapter under plain g++, the restatement
(tests/keyframe_culling_ref.py) against a brute-force triple loop and a case worked out by hand on small tables, and the conditions the
scenes of tests/test_gpu_keyframe_culling.py must meet, asserted on the restatement of the backend alone."""
import ctypes as C
import os
import re
import subprocess
import numpy as np
import pytest
import backend_ref as br
from compaction_scenes import crosses_blocks
import covisibility_ref as cr
import keyframe_culling_ref as kr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "dynamic-visual-slam_amd", "lib")
NAMES = ["dvs_cull_default_params", "dvs_backend_cull_keyframes"]


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
                 'int main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(dvs_cull_params), offsetof(dvs_cull_params, drop_orphans),\n'
                 '  offsetof(dvs_cull_params, local), sizeof(dvs_cull_result), offsetof(dvs_cull_result, n_culled), offsetof(dvs_cull_result, n_landmarks_removed));\n'
                 '  return 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), src, "-o", exe])
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [32, 24, 12, 32, 12, 20]
    assert C.sizeof(B.CullParams) == 32 and B.CullParams.drop_orphans.offset == 24 and B.CullParams.local.offset == 12
    assert C.sizeof(B.CullResult) == 32 and B.CullResult.n_culled.offset == 12 and B.CullResult.n_landmarks_removed.offset == 20
    p = B.cull_params()
    assert {k: getattr(p, k) for k in kr.DEFAULTS} == kr.DEFAULTS and p.local == 0 and p.reserved == 0
    with pytest.raises(TypeError):
        B.cull_params(min_observres=3)
    with pytest.raises(TypeError):
        B.cull_params(reserved=1)


def test_null_and_argument_errors_come_before_any_handle_work(hiplib):
    from dvslam_amd import backend as B
    B._bind(hiplib)
    n, r = C.c_int32(), B.CullResult()
    p = B.cull_params()
    assert hiplib.dvs_backend_cull_keyframes(None, 1, C.byref(p), None, 0, 0, C.byref(r), 0, None, None, None, None, C.byref(n)) == -6
    assert b"bad argument" in hiplib.dvs_last_error()
    hiplib.dvs_cull_default_params(None)
    # the parameters are judged before the handle is read: any non-null address does for one
    fake = C.create_string_buffer(64)
    h = C.cast(fake, C.c_void_p)
    assert hiplib.dvs_backend_cull_keyframes(h, 1, C.byref(p), None, 0, 0, C.byref(r), 0, None, None, None, None, None) == -6           # no n_kf
    assert hiplib.dvs_backend_cull_keyframes(h, 1, C.byref(p), None, 0, 0, C.byref(r), -1, None, None, None, None, C.byref(n)) == -6   # cap_kf < 0
    assert hiplib.dvs_backend_cull_keyframes(h, 1, C.byref(p), None, -1, 0, C.byref(r), 0, None, None, None, None, C.byref(n)) == -6   # n_protected < 0
    assert hiplib.dvs_backend_cull_keyframes(h, 1, C.byref(p), None, 2, 0, C.byref(r), 0, None, None, None, None, C.byref(n)) == -6    # ids announced, none given
    for bad in (dict(min_observers=0), dict(redundancy_percent=-1), dict(redundancy_percent=100), dict(min_weight=0), dict(keep_recent=-1), dict(max_cull=-1)):
        q = B.cull_params(**bad)
        assert hiplib.dvs_backend_cull_keyframes(h, 1, C.byref(q), None, 0, 1, C.byref(r), 0, None, None, None, None, C.byref(n)) == -6, bad
        assert b"bad argument" in hiplib.dvs_last_error()
    assert fake.raw == bytes(64)


def test_adapter_header_compiles_with_plain_gpp(hiplib, tmp_path):
    src = os.path.join(str(tmp_path), "adapter.cpp"); exe = os.path.join(str(tmp_path), "adapter")
    with open(src, "w") as fh:
        fh.write('#include <cstdio>\n#include "dvslam/keyframe_culling.hpp"\n'
                 'int main() {\n  dvslam::CullParams p;\n'
                 '  std::printf("%d %d %d %d %d %d %d %d\\n", p.min_observers, p.redundancy_percent, p.min_weight, p.local, p.keep_recent, p.max_cull, p.drop_orphans,\n'
                 '              (int)sizeof(dvs_cull_result));\n'
                 '  if (dvs_device_count() < 1) return 3;\n'
                 '  dvs_backend_params bp; dvs_backend_default_params(&bp); bp.fx = bp.fy = 500.0; bp.cx = 320.0; bp.cy = 240.0;\n'
                 '  dvslam::MappingBackend map(bp);\n  dvslam::CullReport r = dvslam::cullKeyframes(map, p, {}, true);\n'
                 '  if (r.result.n_keyframes != 0 || r.result.n_culled != 0 || !r.kf_state.empty() || !r.culled_frame_id.empty()) return 1;\n'
                 '  try { dvslam::cullKeyframes(map, 5, p); } catch (const std::runtime_error&) { return 0; }\n'
                 '  return 1;\n}\n')
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), src, "-o", exe, "-L" + LIBDIR,
                           "-ldvslam_hip", "-Wl,-rpath," + LIBDIR, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode in (0, 3) and out.stdout.split() == ["3", "90", "15", "0", "2", "0", "1", "32"], out.stdout[-2000:] + out.stderr[-2000:]


# ---------------------------------------------------------------------------------------------------- the restatement on hand-made tables
def _tables(frames, lm_ids, rows, counts=None):
    """keyframes with those frame ids, landmarks with those ids, observation rows (frame id, landmark id) in table order: every column the
    getters return.  Observation ids are 100 + row; observation_count is the number of rows naming the landmark unless `counts` says otherwise"""
    nk, nl, no = len(frames), len(lm_ids), len(rows)
    oid = [100 + i for i in range(no)]
    koffs, kids = [0], []
    for f in frames:
        kids += [oid[i] for i, r in enumerate(rows) if r[0] == f]
        koffs.append(len(kids))
    loffs, lids = [0], []
    for l in lm_ids:
        lids += [oid[i] for i, r in enumerate(rows) if r[1] == l]
        loffs.append(len(lids))
    kfs = dict(frame_id=np.array(frames, np.uint64), stamp_ns=np.arange(nk, dtype=np.int64) * 10**9, R=np.tile(np.eye(3), (nk, 1, 1)), t=np.arange(3.0 * nk).reshape(nk, 3),
               obs_offsets=np.array(koffs, np.int64), obs_ids=np.array(kids, np.uint64))
    lms = dict(id=np.array(lm_ids, np.uint64), class_id=np.arange(nl, dtype=np.int32) % 3, xyz=np.arange(3 * nl, dtype=np.float32).reshape(nl, 3),
               desc=np.arange(32 * nl, dtype=np.int64).astype(np.uint8).reshape(nl, 32),
               observation_count=np.array(counts if counts is not None else np.diff(loffs), np.int32), last_seen_ns=np.arange(nl, dtype=np.int64) * 7,
               obs_offsets=np.array(loffs, np.int64), obs_ids=np.array(lids, np.uint64))
    obs = dict(id=np.array(oid, np.uint64), frame_id=np.array([r[0] for r in rows], np.uint64), landmark_id=np.array([r[1] for r in rows], np.uint64),
               px=np.arange(2 * no, dtype=np.float32).reshape(no, 2), desc=np.arange(32 * no, dtype=np.int64).astype(np.uint8).reshape(no, 32)[::-1].copy(),
               class_id=np.arange(no, dtype=np.int32) % 3)
    return kfs, lms, obs


# test_covisibility_cpu.HAND's rows: keyframe 10 names landmark 2 twice and the absent landmark 4; keyframe 13 has no rows; frame 99 is no
# keyframe; landmark 5 is seen by keyframes 11 and 12 only, which both go below: an orphan.  Landmark 8's observation_count is below its rows.
HAND = _tables([10, 11, 12, 13, 14], [1, 2, 3, 5, 8],
               [(10, 1), (10, 2), (10, 2), (10, 3), (10, 4), (11, 1), (11, 2), (11, 5), (12, 1), (12, 3), (12, 5), (12, 5), (12, 8), (14, 2), (14, 8), (99, 1)],
               counts=[4, 4, 2, 3, 0])
CHAIN = _tables([3, 1, 2, 5, 4], [7, 9, 11], [(3, 7), (1, 7), (1, 9), (2, 9), (2, 9), (2, 7), (5, 7), (5, 9), (5, 11), (4, 11), (4, 9)])


def _brute(kfs, lms, obs, P, candidates):
    """the walk as a triple loop: keyframes x landmarks x rows for every count, every time -> (culled indices, R_k under the initial counts)"""
    frames = kfs["frame_id"].tolist(); ids = lms["id"].tolist()
    rows = list(zip(obs["frame_id"].tolist(), obs["landmark_id"].tolist()))

    def sees(k, l):
        return any(f == frames[k] and x == l for f, x in rows)

    def R_of(k, alive):
        n = R = 0
        for l in ids:
            if sees(k, l):
                n += 1
                R += sum(1 for a in alive if a != k and sees(a, l)) >= P["min_observers"]
        return n, R
    alive = list(range(len(frames)))
    first = [R_of(k, alive) for k in range(len(frames))]
    culled = []
    for k in candidates:
        n, R = R_of(k, alive)
        if n >= 1 and 100 * R > P["redundancy_percent"] * n:
            alive.remove(k); culled.append(k)
            if P["max_cull"] and len(culled) == P["max_cull"]:
                break
    return culled, first


@pytest.mark.parametrize("T", [HAND, CHAIN], ids=["hand", "chain"])
def test_walk_equals_a_brute_force_triple_loop(T):
    nkf = len(T[0]["frame_id"])
    differ = 0
    for mo in (1, 2, 3):
        for pct in (0, 50, 60, 74, 75, 99):
            for keep in (0, 1, 2):
                for mc in (0, 1):
                    P = dict(kr.DEFAULTS, min_observers=mo, redundancy_percent=pct, keep_recent=keep, max_cull=mc)
                    d = kr.decide(*T, **P)
                    cand = [k for k in range(1, nkf - keep)]
                    culled, first = _brute(*T, P, cand)
                    assert np.nonzero(d["kf_state"] == kr.CULLED)[0].tolist() == culled, P
                    assert d["kf_observed"].tolist() == [f[0] for f in first] and d["kf_redundant"].tolist() == [f[1] for f in first], P
                    assert d["n_candidates"] == len(cand) and d["n_culled"] == len(culled)
                    assert [int(s) for s in d["kf_state"]] == [kr.PROTECTED if k not in cand else kr.CULLED if k in culled else kr.KEPT for k in range(nkf)]
                    differ += kr.decide(*T, one_shot=True, **P)["kf_state"].tolist() != d["kf_state"].tolist()
    assert differ > 0                                                        # the tables tell the walk from a one-shot test


def test_hand_table_worked_out_by_hand():
    # S = {1,2,3} {1,2,5} {1,3,5,8} {} {2,8}; c = 3, 3, 2, 2, 2 for landmarks 1, 2, 3, 5, 8
    P = dict(min_observers=1, redundancy_percent=60, keep_recent=0)
    d = kr.decide(*HAND, **P)
    assert d["kf_observed"].tolist() == [3, 3, 4, 0, 2] and d["kf_redundant"].tolist() == [3, 3, 4, 0, 2] and d["n_redundant_initial"] == 4
    # 10 is index 0; 11: 3 of 3; then 12: landmark 5 is down to one observer, 3 of 4 is still above 60 %; 13 observes nothing; 14: landmark 8
    # is down to one observer, 1 of 2 is not above 60 %
    assert d["kf_state"].tolist() == [1, 3, 3, 2, 2] and d["culled_frame_id"].tolist() == [11, 12] and d["n_candidates"] == 4 and d["n_culled"] == 2
    assert kr.decide(*HAND, one_shot=True, **P)["kf_state"].tolist() == [1, 3, 3, 2, 3]
    assert kr.decide(*HAND, protected=(12,), **P)["kf_state"].tolist() == [1, 3, 1, 2, 3]          # 12 stays, so 8 keeps two observers and 14 goes
    assert kr.decide(*HAND, max_cull=1, **P)["kf_state"].tolist() == [1, 3, 2, 2, 2]
    assert kr.decide(*HAND, **dict(P, keep_recent=4))["kf_state"].tolist() == [1, 1, 1, 1, 1]
    # local scope around 14 at theta = 1: W[4] = 1 1 1 0 -> 10, 11 and 12 are in scope, 13 is not, 14 itself is protected
    loc = kr.decide(*HAND, 14, min_weight=1, **P)
    assert loc["kf_state"].tolist() == [1, 3, 3, 0, 1] and loc["n_candidates"] == 2
    assert kr.decide(*HAND, 14, min_weight=2, **P)["kf_state"].tolist() == [1, 0, 0, 0, 1]
    rep, kfs, lms, obs = kr.cull(*HAND, **P)
    assert rep["n_observations_removed"] == 8 and rep["n_landmarks_removed"] == 1
    keep = [0, 1, 2, 3, 4, 13, 14, 15]
    assert kfs["frame_id"].tolist() == [10, 13, 14] and kfs["obs_offsets"].tolist() == [0, 5, 5, 7] and kfs["obs_ids"].tolist() == [100, 101, 102, 103, 104, 113, 114]
    assert kfs["t"].tobytes() == HAND[0]["t"][[0, 3, 4]].tobytes() and kfs["stamp_ns"].tolist() == [0, 3 * 10**9, 4 * 10**9]
    assert all(obs[k].tobytes() == HAND[2][k][keep].tobytes() for k in obs) and set(obs) == set(HAND[2])
    # landmark 5 was seen by 11 and 12 only: the orphan.  Counts 4, 4, 2, -, 0 lose 2, 1, 1, -, 1 rows, and 8's stays at 0
    assert lms["id"].tolist() == [1, 2, 3, 8] and lms["observation_count"].tolist() == [2, 3, 1, 0]
    assert lms["obs_offsets"].tolist() == [0, 2, 5, 6, 7] and lms["obs_ids"].tolist() == [100, 115, 101, 102, 113, 103, 114]
    assert all(lms[k].tobytes() == HAND[1][k][[0, 1, 2, 4]].tobytes() for k in ("xyz", "desc", "last_seen_ns", "class_id"))
    rep, kfs, lms, obs = kr.cull(*HAND, drop_orphans=0, **P)
    assert rep["n_landmarks_removed"] == 0 and lms["id"].tolist() == [1, 2, 3, 5, 8] and lms["observation_count"].tolist() == [2, 3, 1, 0, 0]
    assert lms["obs_offsets"].tolist() == [0, 2, 5, 6, 6, 7]
    # a dry run and a call that culls nothing hand the tables back as they are
    rep, kfs, lms, obs = kr.cull(*HAND, do_apply=False, **P)
    assert rep["n_observations_removed"] == 8 and rep["n_landmarks_removed"] == 1 and kfs is HAND[0] and lms is HAND[1] and obs is HAND[2]
    rep, kfs, lms, obs = kr.cull(*HAND)
    assert rep["n_culled"] == 0 and rep["n_observations_removed"] == 0 and rep["n_landmarks_removed"] == 0 and kfs is HAND[0]


def test_parameter_errors():
    for bad in (dict(min_observers=0), dict(redundancy_percent=-1), dict(redundancy_percent=100), dict(min_weight=0), dict(keep_recent=-1), dict(max_cull=-1)):
        with pytest.raises(ValueError):
            kr.decide(*HAND, **bad)
    with pytest.raises(ValueError):
        kr.decide(*HAND, 98)
    with pytest.raises(ValueError):
        kr.decide(*HAND, protected=(10, 98))
    empty = _tables([], [], [])
    d = kr.decide(*empty)
    assert d["n_keyframes"] == 0 and d["n_culled"] == 0 and len(d["kf_state"]) == 0


# ---------------------------------------------------------------------------------------------------- the scenes of the GPU tests
HUB_ID = cr.HUB_FRAME0 + cr.HUB
# (min_observers, protected frame ids, max_cull) at 90 %, keep_recent = 0: index 0 and the hub are all that is ever protected
HUB_SETS = [(3, (), 0), (1, (), 0), (1, (HUB_ID,), 0), (1, (HUB_ID,), 70)]


def _culled(d):
    return np.nonzero(d["kf_state"] == kr.CULLED)[0].tolist()


def test_hub_scene_meets_its_conditions():
    T = cr.tables(cr.scene_ref(cr.hub_scene(), cls=cr.IncidenceRef))
    got = [kr.decide(*T, None, prot, min_observers=mo, max_cull=mc, keep_recent=0) for mo, prot, mc in HUB_SETS]
    shot = kr.decide(*T, one_shot=True, keep_recent=0)
    assert [(d["n_redundant_initial"], d["n_culled"]) for d in got] == [(194, 186), (300, 193), (300, 295), (300, 70)] and shot["n_culled"] == 193
    assert max(d["n_candidates"] for d in got) > 256 and got[1]["n_candidates"] == 299                    # more walked candidates than one trip
    a = got[0]
    assert [sum(a["kf_state"][k] != kr.CULLED for k in c) for c in cr.HUB_CLUSTERS] == [2, 3, 3, 2]
    assert a["kf_state"][cr.HUB] == kr.KEPT and all(a["kf_state"][k] == kr.KEPT for k in cr.HUB_LEAVES)
    leaves = set(cr.HUB_LEAVES)
    assert cr.HUB in _culled(got[1]) and not leaves & set(_culled(got[1]))
    assert got[2]["kf_state"][cr.HUB] == kr.PROTECTED and leaves <= set(_culled(got[2]))                  # the hub's protection flips 103 decisions
    assert _culled(got[3])[-1] == 71 and _culled(got[3]) == _culled(got[2])[:70]
    assert a["kf_observed"][cr.HUB] == 1 + cr.HUB_OWN + cr.HUB_BLOCK > 256
    # local scope around the first member of cluster 0
    loc = kr.decide(*T, cr.HUB_FRAME0 + cr.HUB_CLUSTERS[0][0], min_weight=15)
    assert (loc["kf_state"] >= kr.KEPT).sum() == 65 and loc["n_candidates"] == 65 and loc["n_culled"] == 63 and (loc["kf_state"] == kr.OUT).sum() == 300 - 65 - 3
    # the default apply
    rep, kfs, lms, obs = kr.cull(*T)
    assert rep["n_culled"] == 186 and (rep["n_observations_removed"], len(T[2]["id"])) == (3906, 4858) and rep["n_landmarks_removed"] == 0
    gone = np.isin(T[2]["frame_id"], rep["culled_frame_id"])
    blocks = [gone[b:b + 256] for b in range(0, len(gone), 256)]
    assert len(blocks) == 19 and sum(1 for b in blocks if 0 < b.sum() < len(b)) == 5
    assert (kr.rows_per_landmark(T[1], T[2]) == T[1]["observation_count"]).all() and (kr.rows_per_landmark(lms, obs) == lms["observation_count"]).all()
    assert len(kfs["frame_id"]) == 114 and len(obs["id"]) == 952 and kr.cull(kfs, lms, obs)[0]["n_culled"] == 0          # a second call culls nothing


def test_make_scene_meets_its_conditions():
    T = cr.tables(cr.scene_ref(br.make_scene(), filtered=(br.PERSON,)))
    assert (kr.rows_per_landmark(T[1], T[2]) == T[1]["observation_count"]).all()
    assert kr.decide(*T)["n_culled"] == 0
    P = dict(min_observers=2, redundancy_percent=70)
    rep, kfs, lms, obs = kr.cull(*T, **P)
    assert _culled(rep) == [3, 7] and _culled(kr.decide(*T, one_shot=True, **P)) == [3, 4, 5, 7] and rep["n_landmarks_removed"] == 60
    assert (kr.rows_per_landmark(lms, obs) == lms["observation_count"]).all() and len(lms["id"]) == len(T[1]["id"]) - 60
    # the apply's compactions work across workgroups on both tables (the hub scene removes no landmark: this scene carries the condition)
    assert crosses_blocks(T[1]["id"], lms["id"]) == (True, True) and crosses_blocks(T[2]["id"], obs["id"]) == (True, True)
    rep0, _, lms0, obs0 = kr.cull(*T, drop_orphans=0, **P)
    assert rep0["n_landmarks_removed"] == 0 and (kr.rows_per_landmark(lms0, obs0) == 0).sum() == 60 and obs0["id"].tobytes() == obs["id"].tobytes()
    rec = kr.decide(*T, keep_recent=3, **P)
    assert _culled(rec) == [3] and rec["kf_state"][7] == kr.PROTECTED


def test_fused_scene_meets_its_conditions():
    ref, _ = cr.fused_ref()
    T = cr.tables(ref)
    assert cr.repeated_pairs(*T) > 0 and (kr.rows_per_landmark(T[1], T[2]) == T[1]["observation_count"]).all()
    rep, kfs, lms, obs = kr.cull(*T, min_observers=2, redundancy_percent=70)
    assert _culled(rep) == [2, 4, 7] and rep["n_landmarks_removed"] == 87
    assert (kr.rows_per_landmark(lms, obs) == lms["observation_count"]).all()
    # a culled keyframe named a surviving landmark twice: its observation_count falls by 2 for one keyframe
    gone = set(int(f) for f in rep["culled_frame_id"])
    pairs = [(int(f), int(l)) for f, l in zip(T[2]["frame_id"], T[2]["landmark_id"]) if int(f) in gone]
    twice = set(l for f, l in pairs if pairs.count((f, l)) == 2) & set(int(l) for l in lms["id"])
    assert twice
    before = dict(zip(T[1]["id"].tolist(), T[1]["observation_count"].tolist())); after = dict(zip(lms["id"].tolist(), lms["observation_count"].tolist()))
    assert all(before[l] - after[l] >= 2 for l in twice)


def test_maps_of_one_and_two_keyframes():
    scene = br.make_scene()
    for n in (1, 2):
        T = cr.tables(cr.scene_ref(scene[:n], filtered=(br.PERSON,)))
        for keep in (0, 2):
            d = kr.decide(*T, min_observers=1, redundancy_percent=0, keep_recent=keep)
            assert d["kf_state"].tolist() == ([1] if n == 1 else [1, 3 if keep == 0 else 1]) and d["kf_observed"][0] > 15
