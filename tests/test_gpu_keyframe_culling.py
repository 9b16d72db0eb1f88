"""GPU: keyframe culling (include/dvslam_hip.h "Keyframe culling") against the restatement run on the getters' output of the same handle
(tests/keyframe_culling_ref.py), bit for bit.  The scenes' conditions are asserted without a GPU in tests/test_keyframe_culling_cpu.py; the
few that decide whether a test here checks anything are asserted again on the device's tables.  Every test that calls
MappingBackend.cull_keyframes fails without the feature (no such symbol)."""
import ctypes as C
import numpy as np
import pytest
import backend_ref as br
import covisibility_ref as cr
import keyframe_culling_ref as kr
import loop_closing_ref as lc

pytestmark = pytest.mark.gpu
HUB_ID = cr.HUB_FRAME0 + cr.HUB


def _handle(keyframes, mb=None):
    from dvslam_amd.backend import MappingBackend
    if mb is None:
        mb = MappingBackend(br.FX, br.FY, br.CX, br.CY, filtered=("person",), initial_capacity=64)
        assert mb.intern("person") == br.PERSON and mb.intern("chair") == br.CHAIR and mb.intern("table") == br.TABLE
    for kf in keyframes:
        lc.add(mb, kf)
    return mb


def _fused_handle():
    mb = _handle(br.make_scene())
    assert mb.fuse(cr.FUSED_QUERY, cr.FUSED_ENTRIES, **cr.FUSED_PARAMS)["n_fused"] > 0
    return mb


def _tables(mb):
    """(keyframes, landmarks, observations): the order the restatement takes them"""
    return mb.keyframes(), mb.landmarks(), mb.observations()


def _same(got, want, what):
    assert set(got) == set(want), (what, sorted(got), sorted(want))
    for k in want:
        if np.isscalar(want[k]):
            assert got[k] == want[k], (what, k, got[k], want[k])
            continue
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (what, k)


def _same_tables(got, want, what):
    for name, a, b in zip(("keyframes", "landmarks", "observations"), got, want):
        _same(a, b, (what, name))


def _cull_both(mb, ref_frame_id=None, protected=(), apply=True, what="", **params):
    """the call on the handle and on the restatement of its own tables -> (report, tables before, the restatement's tables after)"""
    T = _tables(mb)
    want, *after = kr.cull(*T, ref_frame_id, protected, do_apply=apply, **params)
    got = mb.cull_keyframes(ref_frame_id, protected, apply, **params)
    _same(got, want, (what, params, "report"))
    _same_tables(_tables(mb), after, (what, params))
    return got, T, after


def _culled(rep):
    return np.nonzero(rep["kf_state"] == kr.CULLED)[0].tolist()


@pytest.fixture(scope="module")
def hub(gpu):
    mb = _handle(cr.hub_scene())
    yield mb
    mb.close()


def test_hub_scene_dry_runs_equal_the_restatement(hub):
    """lists above 256, a segment of 300 views, more than 256 walked candidates, the early stop, the hub's protection flipping 103 decisions,
    and the local scope; a dry run leaves every byte of the three getters"""
    before = _tables(hub)
    reps = []
    for mo, prot, mc in ((3, (), 0), (1, (), 0), (1, (HUB_ID,), 0), (1, (HUB_ID,), 70)):
        got, T, after = _cull_both(hub, None, prot, False, "hub", min_observers=mo, max_cull=mc, keep_recent=0)
        assert all(a is b for a, b in zip(T, after))
        reps.append(got)
    assert [(r["n_redundant_initial"], r["n_culled"]) for r in reps] == [(194, 186), (300, 193), (300, 295), (300, 70)]
    assert reps[0]["kf_observed"][cr.HUB] > 256 and reps[1]["n_candidates"] == 299 and reps[0]["n_observations_removed"] > 0
    assert _culled(reps[0]) != _culled(kr.decide(*before, one_shot=True, keep_recent=0))                   # a one-shot test fails here
    leaves = set(cr.HUB_LEAVES)
    assert cr.HUB in _culled(reps[1]) and not leaves & set(_culled(reps[1])) and leaves <= set(_culled(reps[2])) and _culled(reps[3])[-1] == 71
    loc, _, _ = _cull_both(hub, cr.HUB_FRAME0 + cr.HUB_CLUSTERS[0][0], (), False, "hub local", min_weight=15)
    assert (loc["n_candidates"], loc["n_culled"]) == (65, 63) and (loc["kf_state"] == kr.OUT).sum() == 232
    again = hub.cull_keyframes(cr.HUB_FRAME0 + cr.HUB_CLUSTERS[0][0], (), False, min_weight=15)
    _same(again, loc, "second call")
    _same_tables(_tables(hub), before, "dry runs")


def test_hub_scene_default_apply(gpu):
    from dvslam_amd import DvsError
    mb = _handle(cr.hub_scene())
    counts = mb.counts()
    rep, before, after = _cull_both(mb, what="hub apply")
    assert rep["n_culled"] == 186 and (rep["n_observations_removed"], len(before[2]["id"])) == (3906, 4858) and rep["n_landmarks_removed"] == 0
    gone = np.isin(before[2]["frame_id"], rep["culled_frame_id"])
    assert sum(1 for b in range(0, len(gone), 256) if 0 < gone[b:b + 256].sum() < len(gone[b:b + 256])) == 5       # blocks of 256 rows with both kinds
    now = mb.counts()
    assert (now["n_keyframes"], now["n_observations"], now["n_landmarks"]) == (114, 952, counts["n_landmarks"])
    assert (now["next_observation_id"], now["next_landmark_id"]) == (counts["next_observation_id"], counts["next_landmark_id"])
    T = _tables(mb)
    assert (kr.rows_per_landmark(T[1], T[2]) == T[1]["observation_count"]).all()
    _same(mb.covisibility(1), cr.graph(*T, 1), "graph of the culled map")
    rep2, _, _ = _cull_both(mb, what="second call")
    assert rep2["n_culled"] == 0 and rep2["n_keyframes"] == 114
    _same_tables(_tables(mb), T, "second call")
    # the handle goes on: a kept frame id is still taken, a culled one is free again, and the sliding window finds the renumbered rows
    kf = dict(cr.hub_scene()[5])
    kept, culled = int(T[0]["frame_id"][5]), int(rep["culled_frame_id"][0])
    with pytest.raises(DvsError):
        lc.add(mb, dict(kf, frame_id=kept))
    res = lc.add(mb, dict(kf, frame_id=culled, stamp=(900, 0)))
    assert res["n_kept"] == len(kf["px"]) and res["n_associated"] == res["n_kept"] and res["first_observation_id"] == counts["next_observation_id"]
    K, L, O = _tables(mb)
    assert K["frame_id"].tolist() == T[0]["frame_id"].tolist() + [culled] and len(O["id"]) == 952 + res["n_kept"]
    w = mb.window()
    last = K["frame_id"][-5:]
    rows = np.isin(O["frame_id"], last)
    assert w["kf_frame_id"].tolist() == last.tolist() and w["obs_frame_id"].tobytes() == O["frame_id"][rows].tobytes()
    assert w["obs_px"].tobytes() == O["px"][rows].tobytes() and w["obs_landmark_id"].tobytes() == O["landmark_id"][rows].tobytes()
    want = cr.local_window(K, L, O, culled)
    want.pop("kf_index")
    _same(mb.local_window(culled), want, "local window of the culled map")
    mb.close()


def test_make_scene_orphans_and_keep_recent(gpu):
    P = dict(min_observers=2, redundancy_percent=70)
    mb = _handle(br.make_scene())
    rep, _, _ = _cull_both(mb, apply=False, what="default")
    assert rep["n_culled"] == 0 and rep["n_redundant_initial"] == 0
    rec, _, _ = _cull_both(mb, apply=False, what="keep_recent", keep_recent=3, **P)
    assert _culled(rec) == [3] and rec["kf_state"][7] == kr.PROTECTED
    rep, before, after = _cull_both(mb, what="orphans leave", **P)
    assert _culled(rep) == [3, 7] and rep["culled_frame_id"].tolist() == [103, 107] and rep["n_landmarks_removed"] == 60
    assert len(after[1]["id"]) == len(before[1]["id"]) - 60 and (kr.rows_per_landmark(*_tables(mb)[1:]) == mb.landmarks()["observation_count"]).all()
    assert _culled(kr.decide(*before, one_shot=True, **P)) == [3, 4, 5, 7]
    mb.close()
    mb = _handle(br.make_scene())
    rep, before, after = _cull_both(mb, what="orphans stay", drop_orphans=0, **P)
    K, L, O = _tables(mb)
    assert _culled(rep) == [3, 7] and rep["n_landmarks_removed"] == 0 and len(L["id"]) == len(before[1]["id"])
    rows = kr.rows_per_landmark(L, O)
    assert (rows == 0).sum() == 60 and (L["observation_count"] == rows).all() and (np.diff(L["obs_offsets"]) == rows).all()
    mb.close()


def test_fused_scene_counts_fall_by_two(gpu):
    mb = _fused_handle()
    rep, before, after = _cull_both(mb, what="fused", min_observers=2, redundancy_percent=70)
    assert _culled(rep) == [2, 4, 7] and rep["n_landmarks_removed"] == 87 and cr.repeated_pairs(*before) > 0
    K, L, O = _tables(mb)
    assert (kr.rows_per_landmark(L, O) == L["observation_count"]).all()
    gone = set(int(f) for f in rep["culled_frame_id"])
    pairs = [(int(f), int(l)) for f, l in zip(before[2]["frame_id"], before[2]["landmark_id"]) if int(f) in gone]
    twice = set(l for f, l in pairs if pairs.count((f, l)) == 2) & set(int(l) for l in L["id"])
    was = dict(zip(before[1]["id"].tolist(), before[1]["observation_count"].tolist())); now = dict(zip(L["id"].tolist(), L["observation_count"].tolist()))
    assert twice and all(was[l] - now[l] >= 2 for l in twice)
    mb.close()


def test_pose_graph_and_bundle_adjustment_after_an_apply(gpu):
    """the culled map through the calls that read the keyframe list: the pose graph's odometry chain, then global and local BA, each the
    restated assembly of the culled tables solved directly"""
    import global_ba_ref as gr
    from dvslam_amd import BAProblem
    mb = _handle(br.make_scene())
    rep, _, _ = _cull_both(mb, what="make_scene", min_observers=2, redundancy_percent=70)
    K, L, O = _tables(mb)
    nkf = len(K["frame_id"])
    assert rep["n_culled"] == 2 and nkf == 8
    g = mb.build_pose_graph([], lc.ODO_W)
    assert len(g["ei"]) == nkf - 1 and g["ei"].tolist() == list(range(nkf - 1)) and g["ej"].tolist() == list(range(1, nkf)) and g["R"].tobytes() == K["R"].tobytes()
    P, left_out, used = gr.assemble(K, L, O, br.FX, br.FY, br.CX, br.CY)
    out = mb.global_bundle_adjust()
    s = out["summary"].ba
    assert (out["n_cameras"], out["n_landmarks"], out["n_observations"], out["n_left_out"]) == (nkf, P["L"], len(P["cam_idx"]), left_out)
    direct = BAProblem(P)
    sg = direct.solve_global().ba
    assert (sg.termination, sg.initial_cost, sg.final_cost, sg.num_iterations) == (s.termination, s.initial_cost, s.final_cost, s.num_iterations)
    K2, L2, O2 = _tables(mb)
    assert K2["frame_id"].tolist() == K["frame_id"].tolist() and not set(K2["frame_id"].tolist()) & set(rep["culled_frame_id"].tolist())
    if s.termination == 0:
        q, t, X = direct.parameters()
        for k in range(1, nkf):
            R, tt = gr.pose_to_rt(q[k], t[k])
            assert K2["R"][k].tobytes() == R.tobytes() and K2["t"][k].tobytes() == tt.tobytes(), k
        assert L2["xyz"][used].tobytes() == X[used].astype(np.float32).tobytes()
    else:
        _same_tables((K2, L2, O2), (K, L, O), "a global BA that did not converge")
    frame = int(K2["frame_id"][-1])
    w = cr.local_window(K2, L2, O2, frame)
    PL, usedl, dropped = cr.local_ba_problem(w, br.FX, br.FY, br.CX, br.CY)
    lo = mb.local_bundle_adjust(frame)
    sl = BAProblem(PL).solve_device(20, 1e-6, 1e-10, 1e-8)
    assert {k: lo[k] for k in lo if k != "summary"} == dict(n_cameras=PL["K"], n_fixed=int(w["kf_fixed"].sum()), n_landmarks=PL["L"], n_observations=len(PL["cam_idx"]),
                                                            n_left_out=w["n_left_out"], n_dropped=dropped)
    assert (lo["summary"].termination, lo["summary"].initial_cost, lo["summary"].final_cost, lo["summary"].num_iterations) == \
        (sl.termination, sl.initial_cost, sl.final_cost, sl.num_iterations)
    assert mb.keyframes()["frame_id"].tolist() == K["frame_id"].tolist()
    mb.close()


def test_errors_leave_the_map_untouched(gpu):
    from dvslam_amd import DvsError, backend as B
    mb = _handle(br.make_scene())
    before = _tables(mb)
    frame = int(before[0]["frame_id"][-1])
    P = dict(min_observers=2, redundancy_percent=70)
    for bad in (dict(min_observers=0), dict(redundancy_percent=-1), dict(redundancy_percent=100), dict(min_weight=0), dict(keep_recent=-1), dict(max_cull=-1)):
        for ref in (None, frame):
            with pytest.raises(DvsError) as e:
                mb.cull_keyframes(ref, **dict(P, **bad))
            assert e.value.code == -6, bad
    for ref, prot in ((None, (100, 77)), (77, ()), (frame, (77,))):
        with pytest.raises(DvsError) as e:
            mb.cull_keyframes(ref, prot, **P)
        assert e.value.code == -6
    with pytest.raises(TypeError):
        mb.cull_keyframes(min_observres=2)
    with pytest.raises(TypeError):
        mb.cull_keyframes(local=1)
    assert mb.cull_keyframes(None, (), False, **P)["n_culled"] == 2          # an unknown ref_frame_id is not read in global scope: 0 is no frame of the map
    # count-then-capacity: *n_kf is set, nothing is applied
    L = mb._L
    p = B.cull_params(**P)
    r, n = B.CullResult(), C.c_int32()
    state = np.zeros(4, np.uint8)
    assert L.dvs_backend_cull_keyframes(mb._h, 0, C.byref(p), None, 0, 1, C.byref(r), 4, None, None, None, B.ptr(state), C.byref(n)) == -3
    assert n.value == 10 and r.n_culled == 0 and not state.any()
    assert L.dvs_backend_cull_keyframes(mb._h, 0, C.byref(p), None, 0, 0, C.byref(r), 0, None, None, None, None, C.byref(n)) == 0     # no array: counts only
    assert (n.value, r.n_keyframes, r.n_culled, r.n_landmarks_removed) == (10, 10, 2, 60)
    _same_tables(_tables(mb), before, "errors")
    mb.close()


def test_small_and_empty_maps(gpu):
    from dvslam_amd.backend import MappingBackend
    mb = MappingBackend(br.FX, br.FY, br.CX, br.CY)
    rep = mb.cull_keyframes()
    assert all(rep[k] == 0 for k in rep if np.isscalar(rep[k])) and all(len(rep[k]) == 0 for k in rep if not np.isscalar(rep[k]))
    mb.close()
    scene = br.make_scene()
    for n in (1, 2):
        mb = _handle(scene[:n])
        for ref in (None, 100):
            _cull_both(mb, ref, (), False, f"{n} keyframes", min_weight=1)
        rep, before, after = _cull_both(mb, what=f"{n} keyframes", min_observers=1, redundancy_percent=0, keep_recent=0)
        assert _culled(rep) == ([] if n == 1 else [1]) and rep["kf_state"][0] == kr.PROTECTED and mb.counts()["n_keyframes"] == 1
        if n == 2:
            assert rep["n_landmarks_removed"] > 0 and rep["n_observations_removed"] == len(before[2]["id"]) - len(after[2]["id"]) > 0
            assert set(after[2]["frame_id"].tolist()) == {100}
        mb.close()


def test_one_handle_big_small_big(gpu):
    """the new row groups sized by a small map, outgrown by a big one, reused by a small one and by a big one again, each call against the
    restatement"""
    scene = br.make_scene()
    P = dict(min_observers=2, redundancy_percent=70)
    mb = _handle(scene[:1])
    sizes = []
    for following in (scene, scene[:2], scene):
        K, L, O = _tables(mb)
        sizes.append((len(K["frame_id"]), len(L["id"]), len(O["id"])))
        _cull_both(mb, int(K["frame_id"][-1]), (), False, "local", min_weight=1, **P)
        _cull_both(mb, what="global", keep_recent=0, min_observers=1, redundancy_percent=50)
        mb.reset()
        _handle(following, mb)
    K, L, O = _tables(mb)
    sizes.append((len(K["frame_id"]), len(L["id"]), len(O["id"])))
    rep, _, _ = _cull_both(mb, what="big again", **P)
    assert _culled(rep) == [3, 7]
    # the groups sized at one keyframe (the largest rule is half to spare plus 64) are outgrown by the whole scene
    assert sizes[1][0] == 10 and all(b > 1.5 * a + 64 for a, b in zip(sizes[0][1:], sizes[1][1:])) and sizes[2][0] == 2 and sizes[3] == sizes[1], sizes
    mb.close()
