"""GPU: landmark tracking statistics and landmark culling (include/dvslam_hip.h "Landmark culling") against the restatement
(tests/landmark_culling_ref.py) run on the getters' output of the same handle, bit for bit throughout.  The recording's expectation is
fed with the device's own matches and per-landmark records, so the record kernel is tested apart from the refinement's floating point.
The scenes' conditions are asserted without a GPU in tests/test_landmark_culling_cpu.py.  Every test here fails without the feature (no
such symbols)."""
import numpy as np
import pytest
import backend_ref as br
import covisibility_ref as cr
import landmark_culling_ref as lcr
import landmark_refresh_ref as lr
import loop_closing_ref as lc
import map_track_ref as mr

pytestmark = pytest.mark.gpu
STAT_KEYS = ("id", "visible", "found", "n_views", "age_kf")


def _handle(keyframes, hooks=False):
    """hooks: every call of the handle goes through the library with the test hooks, as the tracker's whose records are read"""
    from dvslam_amd import backend as B, _lib
    keep = B.lib
    if hooks:
        B.lib = _lib.test_lib
    try:
        mb = B.MappingBackend(br.FX, br.FY, br.CX, br.CY, filtered=("person",), initial_capacity=64)
    finally:
        B.lib = keep
    assert mb.intern("person") == br.PERSON and mb.intern("chair") == br.CHAIR and mb.intern("table") == br.TABLE
    for kf in keyframes:
        lc.add(mb, kf)
    return mb


def _tracker(P=None, hooks=True):
    from dvslam_amd import map_track as M
    P = P or lcr.track_params()
    p = M.default_params(P.rows, P.cols, P.fx, P.fy, P.cx, P.cy, level_sigma2=P.level_sigma2, **{k: getattr(P, k) for k in mr.DEFAULTS if k != "n_levels"})
    return M.MapTracker(p, hooks=hooks)


def _dev(a):
    from dvslam_amd._lib import DeviceBuffer
    a = np.ascontiguousarray(a)
    return DeviceBuffer(max(a.nbytes, 64)).upload(a)


def _tables(mb):
    return mb.keyframes(), mb.landmarks(), mb.observations()


def _ref(mb):
    return lcr.ref_from_tables(*_tables(mb), mb.counts())


def _same(got, want, what):
    assert set(got) == set(want), what
    for k in want:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (what, k)


def _same_map(mb, ref, what):
    _same(mb.landmarks(), ref.landmark_table(), (what, "landmarks"))
    _same(mb.observations(), ref.observation_table(), (what, "observations"))
    _same(mb.keyframes(), ref.keyframe_table(), (what, "keyframes"))
    c = mb.counts()
    assert (c["n_landmarks"], c["n_observations"], c["n_keyframes"], c["next_observation_id"], c["next_landmark_id"]) == \
        (len(ref.landmark_table()["id"]), len(ref.obs), len(ref.kfs), ref.next_obs, ref.next_lm), what


def _stats(mb):
    s = mb.landmark_stats()
    return {k: s[k] for k in STAT_KEYS}, s["n_frames_recorded"]


def _stats_dict(mb):
    s = mb.landmark_stats()
    return {int(i): [int(v), int(f)] for i, v, f in zip(s["id"], s["visible"], s["found"])}


def _same_stats(mb, ref, stats, what):
    _same(_stats(mb)[0], lcr.stats_table(ref, stats), (what, "statistics"))


def _record_expected(stats, mt, ids, res):
    """the restatement's record fed with the device's own records and matches of the call that just ran"""
    rec = mt.landmark_records(); _, kp_id, _, inl = mt.matches()
    assert len(rec) == len(ids)
    lcr.record(stats, ids, rec["visible"], kp_id, inl, res["status"])
    return rec


# ---------------------------------------------------------------------------------------------------- 1, 2: recording
@pytest.mark.parametrize("n_lm", [255, 256, 257, 513])
def test_recording_by_construction_and_status_gates(gpu, n_lm):
    S = lcr.record_scene(n_lm)
    mb, mt = _handle([S["kf"]], hooks=True), _tracker()
    L = mb.landmarks()
    assert len(L["id"]) == n_lm
    ref = _ref(mb)
    kind = S["kind"]
    d_k, d_d = _dev(S["kps"]), _dev(S["kdesc"])
    n_kp = len(S["kps"])
    zero, n0 = _stats(mb)
    assert not zero["visible"].any() and not zero["found"].any() and n0 == 0 and (zero["n_views"] == 1).all() and (zero["age_kf"] == 0).all()
    # the switch off: a status 0 call leaves the statistics byte-identical
    res = mb.track_frame(mt, d_k, d_d, n_kp, S["R"], S["t"])
    assert res["status"] == mr.OK
    _same(_stats(mb)[0], zero, "switch off")
    mb.set_tracking_stats(True)
    # FEW_MATCHES (too few keypoints) and FEW_INLIERS (the prior moved off onto the decoys) record nothing
    few = mb.track_frame(mt, d_k, d_d, 6, S["R"], S["t"])
    assert few["status"] == mr.FEW_MATCHES
    _same(_stats(mb)[0], zero, "FEW_MATCHES")
    off = mb.track_frame(mt, d_k, d_d, n_kp, S["R"], S["t_moved"])
    assert off["status"] == mr.FEW_INLIERS and off["n_matches"] == lcr.N_DECOYS and 0 < off["n_inliers"] < 10, off
    assert mt.landmark_records()["visible"].sum() > 0
    _same(_stats(mb)[0], zero, "FEW_INLIERS")
    assert _stats(mb)[1] == 0
    # one accepted frame
    stats = lcr.align(ref, {})
    res = mb.track_frame(mt, d_k, d_d, n_kp, S["R"], S["t"])
    assert res["status"] == mr.OK and res["n_inliers"] == (kind == lcr.KIND_A).sum() == res["n_matches"]
    _record_expected(stats, mt, L["id"], res)
    got, nrec = _stats(mb)
    _same(got, lcr.stats_table(ref, stats), "one frame")
    assert nrec == 1
    for k, want in ((lcr.KIND_A, (1, 1)), (lcr.KIND_B, (1, 0)), (lcr.KIND_C, (0, 0))):
        assert (got["visible"][kind == k] == want[0]).all() and (got["found"][kind == k] == want[1]).all(), k
    # a second frame adds; a row at INT32_MAX is left alone; the setter and the clear
    a = L["id"][kind == lcr.KIND_A]
    mb.set_landmark_stats([a[0], a[1]], [lcr.INT32_MAX, lcr.INT32_MAX - 1], [5, 5])
    stats[int(a[0])] = [lcr.INT32_MAX, 5]; stats[int(a[1])] = [lcr.INT32_MAX - 1, 5]
    res = mb.track_frame(mt, d_k, d_d, n_kp, S["R"], S["t"])
    _record_expected(stats, mt, L["id"], res)
    assert stats[int(a[0])] == [lcr.INT32_MAX, 5] and stats[int(a[1])] == [lcr.INT32_MAX, 6] and stats[int(a[2])] == [2, 2]
    _same_stats(mb, ref, stats, "second frame")
    assert _stats(mb)[1] == 2
    _same_map(mb, ref, "tracking never touches the map")
    mb.clear_landmark_stats()
    _same(_stats(mb)[0], zero, "cleared")
    assert _stats(mb)[1] == 0
    d_k.free(); d_d.free(); mt.close(); mb.close()


# ---------------------------------------------------------------------------------------------------- 3: local and gated
def _frame_of(kf, rng):
    """the keypoints a keyframe of make_scene() would give the tracker: its pixels in another order, five bits of every descriptor flipped"""
    n = len(kf["px"])
    perm = rng.permutation(n)
    kps = mr.keypoints(kf["px"][perm].astype(np.float32))
    kd = kf["desc"][perm].copy()
    for k in range(n):
        for b in rng.choice(256, 5, replace=False):
            kd[k, b >> 3] ^= np.uint8(1 << (b & 7))
    return kps, kd


def test_local_tracking_records_on_the_ids_of_the_local_map(gpu):
    scene = br.make_scene()
    mb, mt = _handle(scene, hooks=True), _tracker()
    T = _tables(mb)
    ref = _ref(mb)
    kf = scene[-1]
    kps, kd = _frame_of(kf, np.random.default_rng(9))
    d_k, d_d = _dev(kps), _dev(kd)
    R0, t0 = np.diag([-1.0, -1.0, 1.0]), np.asarray(kf["t"], np.float64)
    cp = dict(max_neighbours=3)
    frame = int(T[0]["frame_id"][-1])
    _, _, ids = cr.local_map(*T, frame, **cp)
    all_ids = T[1]["id"].astype(np.int64)
    assert 0 < len(ids) < len(all_ids)
    rows = np.searchsorted(all_ids, ids)
    assert (rows != np.arange(len(ids))).any()                               # U's rows are not the table's rows: the id decides
    # non-zero counters everywhere first, so that "unchanged" is about values
    base = {int(i): [7 + int(i) % 5, int(i) % 3] for i in all_ids}
    mb.set_landmark_stats(all_ids, [base[int(i)][0] for i in all_ids], [base[int(i)][1] for i in all_ids])
    mb.set_tracking_stats(True)
    res = mb.track_frame_local(mt, frame, d_k, d_d, len(kps), R0, t0, **cp)
    assert res["status"] == mr.OK and res["n_inliers"] >= 40, res
    stats = {k: list(v) for k, v in base.items()}
    rec = _record_expected(stats, mt, ids, res)
    assert rec["visible"].sum() > 40 and not rec["visible"].all()
    _same_stats(mb, ref, stats, "local")
    outside = np.setdiff1d(all_ids, ids)
    assert len(outside) > 0 and all(stats[int(i)] == base[int(i)] for i in outside)
    assert sum(stats[int(i)] != base[int(i)] for i in ids) == rec["visible"].sum()
    _same_map(mb, ref, "local tracking never touches the map")
    d_k.free(); d_d.free(); mt.close(); mb.close()


def test_gated_tracking_does_not_count_a_gated_out_landmark(gpu):
    kfs, q = lr.wall_scene()
    mb, mt = _handle(kfs, hooks=True), _tracker(lr.track_params())
    T = _tables(mb)
    ref = _ref(mb)
    ids = T[1]["id"]
    back = mb.landmark_geometry()["normal"][:, 2] < 0
    assert back.sum() == lr.WALL_N
    d_k, d_d = _dev(q["kps"]), _dev(q["kdesc"])
    mb.set_tracking_stats(True)
    stats = lcr.align(ref, {})
    res = mb.track_frame_gated(mt, d_k, d_d, len(q["kps"]), q["R"], q["t"])
    assert res["status"] == mr.OK and mt.gate_counts().tolist() == [0, 0, lr.WALL_N, 0]
    rec = _record_expected(stats, mt, ids, res)
    assert not rec["visible"][back].any() and rec["visible"][~back].all()
    _same_stats(mb, ref, stats, "gated")
    got = _stats(mb)[0]
    assert not got["visible"][back].any() and (got["visible"][~back] == 1).all() and (got["found"] <= got["visible"]).all()
    # the plain call sees them
    res = mb.track_frame(mt, d_k, d_d, len(q["kps"]), q["R"], q["t"])
    rec = _record_expected(stats, mt, ids, res)
    assert res["status"] == mr.OK and rec["visible"].all()
    _same_stats(mb, ref, stats, "plain after gated")
    got = _stats(mb)[0]
    assert (got["visible"][back] == 1).all() and (got["visible"][~back] == 2).all()
    d_k.free(); d_d.free(); mt.close(); mb.close()


# ---------------------------------------------------------------------------------------------------- 4: alignment
def _set_all(mb):
    ids = mb.landmarks()["id"]
    base = {int(i): [10 + int(i) % 7, int(i) % 4] for i in ids}
    mb.set_landmark_stats(ids, [base[int(i)][0] for i in ids], [base[int(i)][1] for i in ids])
    assert _stats_dict(mb) == base
    return base


def _aligned(mb, base, what, min_removed=1, new=False):
    """after an operation on the map: survivors unchanged, removed ids gone, new ids 0 / 0 -> the ids that left"""
    now = _stats_dict(mb)
    ids = [int(i) for i in mb.landmarks()["id"]]
    assert sorted(now) == ids, what
    assert all(now[i] == base.get(i, [0, 0]) for i in ids), what
    gone = sorted(set(base) - set(ids))
    assert len(gone) >= min_removed and (any(i not in base for i in ids) == new), what
    if gone:
        assert gone[0] < max(ids), (what, "rows in the middle leave")
    return gone


def test_alignment_follows_the_map_by_id(gpu):
    scene = br.make_scene()
    mb = _handle(scene[:6])
    base = _set_all(mb)
    lc.add(mb, scene[6])
    _aligned(mb, base, "add_keyframe", min_removed=0, new=True)
    base = _set_all(mb)
    rep = mb.cull_keyframes(apply=True, min_observers=1, redundancy_percent=30, drop_orphans=1)
    assert rep["n_culled"] > 0 and rep["n_landmarks_removed"] > 0, rep
    _aligned(mb, base, "cull_keyframes")
    base = _set_all(mb)
    removed = mb.prune((10 + 3 * 4 + 21, 0))                                 # seen once, by a keyframe that is 20 s old
    assert removed[0] > 0
    _aligned(mb, base, "prune")
    mb.reset()
    assert _stats(mb)[0]["id"].size == 0
    for kf in scene[:2]:
        lc.add(mb, kf)
    now = _stats_dict(mb)
    assert now and all(v == [0, 0] for v in now.values())                    # reset emptied the statistics: ids 0, 1, .. come back with no counters
    mb.close()
    # fusion: the survivor keeps its own counters, the removed id's are dropped
    mb = _handle(scene)
    base = _set_all(mb)
    out = mb.fuse(cr.FUSED_QUERY, cr.FUSED_ENTRIES, **cr.FUSED_PARAMS)
    assert out["n_fused"] > 0
    gone = _aligned(mb, base, "fuse")
    assert sorted(gone) == sorted(int(i) for i in out["pairs"][1])
    now = _stats_dict(mb)
    assert all(now[int(s)] == base[int(s)] for s in out["pairs"][0])
    mb.close()


# ---------------------------------------------------------------------------------------------------- 5: threshold edges
def _cull_both(mb, ref, stats, what, apply=False, **params):
    """the call on the handle and on the restatement, which holds the handle's own map; -> the device's report"""
    want = lcr.cull(ref, stats, do_apply=apply, **params)
    got = mb.cull_landmarks(apply=apply, **params)
    for k in want:
        if isinstance(want[k], np.ndarray):
            assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), (what, k, got[k], want[k])
        else:
            assert got[k] == want[k], (what, k, got[k], want[k])
    _same_map(mb, ref, what)
    _same_stats(mb, ref, stats, what)
    return got


def test_threshold_edges(gpu):
    from dvslam_amd import DvsError
    scene = br.make_scene()
    mb = _handle(scene[:5])
    rep = mb.cull_keyframes(None, [int(kf["frame_id"]) for kf in scene[:5] if kf["frame_id"] != scene[1]["frame_id"]], True, min_observers=1, redundancy_percent=0,
                            keep_recent=0, drop_orphans=0)
    assert rep["n_culled"] == 1 and rep["n_landmarks_removed"] == 0
    ref = _ref(mb)
    tab = lcr.stats_table(ref, {})
    ids, n, age = tab["id"], tab["n_views"], tab["age_kf"]
    lonely = np.flatnonzero(n == 0)
    assert len(lonely) > 0 and (age[lonely] == -1).all()                     # no valid view: created by the keyframe that was culled
    off = dict(found_ratio_pct=0, weak_age_kf=-1)
    got = _cull_both(mb, ref, {}, "both rules off", **off)
    assert got["n_by_ratio"] == got["n_weak"] == 0 and len(got["culled_id"]) == 0
    # rule F at its edges: 25 % of 8 is 2
    a, b, c, d = (int(ids[k]) for k in (3, 4, 5, 6))
    stats = {a: [8, 2], b: [8, 1], c: [3, 0], d: [4, 0]}
    mb.set_landmark_stats([a, b, c, d], [8, 8, 3, 4], [2, 1, 0, 0])
    got = _cull_both(mb, ref, stats, "F", weak_age_kf=-1)
    assert got["culled_id"].tolist() == [b, d] and got["culled_reason"].tolist() == [1, 1]     # equality stays; visible == min_visible - 1 stays
    got = _cull_both(mb, ref, stats, "F off", **off)
    assert len(got["culled_id"]) == 0
    got = _cull_both(mb, ref, stats, "F at 100 %", found_ratio_pct=100, min_visible=1, weak_age_kf=-1)
    assert got["culled_id"].tolist() == [a, b, c, d]
    # rule W at its edges, on a landmark with views
    s = int(np.flatnonzero((n >= 2) & (age >= 1))[0])
    L = int(ids[s])
    for params, goes in ((dict(weak_age_kf=int(age[s]), weak_max_views=int(n[s])), True), (dict(weak_age_kf=int(age[s]) + 1, weak_max_views=int(n[s])), False),
                         (dict(weak_age_kf=int(age[s]), weak_max_views=int(n[s]) - 1), False)):
        got = _cull_both(mb, ref, stats, ("W", params), found_ratio_pct=0, **params)
        assert (L in got["culled_id"].tolist()) == goes, params
        assert not np.isin(ids[lonely], got["culled_id"]).any()              # never weak without a valid view, whatever n <= weak_max_views says
    got = _cull_both(mb, ref, stats, "W wide open", found_ratio_pct=0, weak_age_kf=0, weak_max_views=10 ** 6)
    assert len(got["culled_id"]) == len(ids) - len(lonely)
    # F is counted before W when both hold
    got = _cull_both(mb, ref, stats, "F before W", weak_age_kf=0, weak_max_views=10 ** 6)
    why = dict(zip(got["culled_id"].tolist(), got["culled_reason"].tolist()))
    assert why[b] == why[d] == 1 and why[a] == 2 and got["n_by_ratio"] == 2 and got["n_weak"] == len(ids) - len(lonely) - 2
    for bad in (dict(found_ratio_pct=101), dict(min_visible=0), dict(weak_max_views=-1)):
        with pytest.raises(DvsError):
            mb.cull_landmarks(apply=True, **bad)
    with pytest.raises(DvsError):
        mb.set_landmark_stats([a, b], [1, 1], [2, 0])                        # found > visible
    with pytest.raises(DvsError):
        mb.set_landmark_stats([b, a], [1, 1], [0, 0])                        # ids do not ascend
    with pytest.raises(DvsError):
        mb.set_landmark_stats([a], [-1], [-1])
    mb.set_landmark_stats([10 ** 9], [1], [1])                               # an id the map does not hold is skipped
    _same_map(mb, ref, "nothing was applied")
    _same_stats(mb, ref, stats, "the refused calls changed nothing")
    mb.close()


# ---------------------------------------------------------------------------------------------------- 6: apply
BIG_SCENE = dict(seed=17, npoints=330, nkf=4)    # three keyframes of it: more than 513 landmarks (tests/test_landmark_culling_cpu.py), so "block" needs no larger one


@pytest.fixture(scope="module")
def big_scene():
    return br.make_scene(**BIG_SCENE)


@pytest.mark.parametrize("case", ["edges", "none", "all", "cap", "block", "alternate"])
def test_apply_equals_the_restatement_and_the_map_goes_on(gpu, big_scene, case):
    from dvslam_amd import DvsError
    mb = _handle(big_scene[:3])
    ref = _ref(mb)
    ids = [int(i) for i in mb.landmarks()["id"]]
    assert len(ids) > 513
    base = {i: [9, 3 + i % 5] for i in ids}                                  # found ratio 33 % and more: nobody is in rule F
    # block: a whole 256-row block of the compaction leaves between two that stay; alternate: every block loses half its rows
    marked = dict(edges=[ids[0], ids[255], ids[256], ids[-1]], none=[], all=ids, cap=[ids[0], ids[255], ids[256], ids[-1]], block=ids[256:512], alternate=ids[::2])[case]
    for i in marked:
        base[i] = [9, 2]                                                     # 22 %
    mb.set_landmark_stats(ids, [base[i][0] for i in ids], [base[i][1] for i in ids])
    stats = {k: list(v) for k, v in base.items()}
    if case == "cap":
        before = _tables(mb), _stats(mb)[0]
        with pytest.raises(DvsError):
            mb.cull_landmarks(apply=True, cap=3, weak_age_kf=-1)
        for a, b in zip(_tables(mb), before[0]):
            _same(a, b, "capacity too small: the tables")
        _same(_stats(mb)[0], before[1], "capacity too small: the statistics")
        mb.close()
        return
    got = _cull_both(mb, ref, stats, case, apply=True, weak_age_kf=-1)
    assert got["culled_id"].tolist() == marked and got["n_landmarks_removed"] == len(marked)
    assert (got["n_observations_removed"] > 0) == bool(marked) and (got["n_keyframes_touched"] > 0) == bool(marked)
    # the map goes on: a keyframe and the window, which read every column
    kf = big_scene[3]
    assert lc.add(mb, kf) == lc.add(ref, kf)
    _same_map(mb, ref, (case, "add_keyframe after the cull"))
    _same(mb.window(), ref.window_table(), (case, "window after the cull"))
    _same_stats(mb, ref, stats, (case, "statistics after add_keyframe"))
    mb.close()


# ---------------------------------------------------------------------------------------------------- 7: a moved object
def test_a_moved_object_leaves_the_map(gpu):
    kfs, q = lcr.object_scene()
    mb, mt = _handle(kfs), _tracker(hooks=False)
    ref = _ref(mb)
    obj = lcr.object_ids(ref, q)
    assert len(obj) == lcr.OBJECT_N and len(lcr.landmarks(ref)) == lcr.OBJECT_N + lcr.STATIC_N
    d_k, d_d = _dev(q["kps"]), _dev(q["kdesc"])
    mb.set_tracking_stats(True)
    for _ in range(lcr.DEFAULTS["min_visible"]):
        res = mb.track_frame(mt, d_k, d_d, len(q["kps"]), q["R"], q["t"])
        assert res["status"] == mr.OK and res["n_visible"] == lcr.OBJECT_N + lcr.STATIC_N and res["n_inliers"] == lcr.STATIC_N
    got, nrec = _stats(mb)
    assert nrec == 4 and (got["visible"] == 4).all()
    is_obj = np.isin(got["id"], np.array(sorted(obj), np.uint64))
    assert (got["found"][is_obj] == 0).all() and (got["found"][~is_obj] == 4).all()
    stats = _stats_dict(mb)
    rep = _cull_both(mb, ref, stats, "the object", apply=True)
    assert set(rep["culled_id"].tolist()) == obj and rep["n_by_ratio"] == lcr.OBJECT_N and rep["n_weak"] == 0
    assert rep["n_observations_removed"] == lcr.OBJECT_N * lcr.OBJECT_NKF and rep["n_keyframes_touched"] == lcr.OBJECT_NKF
    mb.set_tracking_stats(False)                                              # the frame below is not recorded: the statistics stay as compared
    after = mb.track_frame(mt, d_k, d_d, len(q["kps"]), q["R"], q["t"])
    assert after["status"] == mr.OK and after["n_visible"] == res["n_visible"] - lcr.OBJECT_N and after["n_inliers"] == lcr.STATIC_N
    again = _cull_both(mb, ref, stats, "nothing left to cull", apply=True)
    assert len(again["culled_id"]) == 0
    d_k.free(); d_d.free(); mt.close(); mb.close()


def test_empty_map(gpu):
    mb = _handle([])
    rep = mb.cull_landmarks()
    assert {k: v for k, v in rep.items() if not isinstance(v, np.ndarray)} == dict(n_landmarks=0, n_by_ratio=0, n_weak=0, n_landmarks_removed=0, n_observations_removed=0,
                                                                                  n_keyframes_touched=0)
    assert len(rep["culled_id"]) == 0 and len(rep["culled_reason"]) == 0
    s = mb.landmark_stats()
    assert all(len(s[k]) == 0 for k in STAT_KEYS) and s["n_frames_recorded"] == 0
    mb.set_landmark_stats([], [], []); mb.clear_landmark_stats(); mb.set_tracking_stats(True)
    mb.close()
