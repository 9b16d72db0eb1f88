"""GPU: landmark refresh (include/dvslam_hip.h "Landmark refresh") against the restatement run on the getters' output of the same handle
(tests/landmark_refresh_ref.py): the selection and the gates bit for bit, the geometry within the forward bound of the longdouble
restatement.  The scenes' conditions are asserted without a GPU in tests/test_landmark_refresh_cpu.py; the few that decide whether a test
here checks anything are asserted again on the device's tables.  Every test here fails without the feature (no such symbols)."""
import numpy as np
import pytest
import backend_ref as br
import covisibility_ref as cr
import landmark_refresh_ref as lr
import loop_closing_ref as lc
import map_track_ref as mr

pytestmark = pytest.mark.gpu


def _handle(keyframes, mb=None):
    from dvslam_amd.backend import MappingBackend
    if mb is None:
        mb = MappingBackend(br.FX, br.FY, br.CX, br.CY, filtered=("person",), initial_capacity=64)
        assert mb.intern("person") == br.PERSON and mb.intern("chair") == br.CHAIR and mb.intern("table") == br.TABLE
    for kf in keyframes:
        lc.add(mb, kf)
    return mb


def _tables(mb):
    return mb.keyframes(), mb.landmarks(), mb.observations()


def _same_tables(got, want, what, but_desc=False):
    for name, a, b in zip(("keyframes", "landmarks", "observations"), got, want):
        assert set(a) == set(b)
        for k in b:
            if but_desc and name == "landmarks" and k == "desc":
                continue
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (what, name, k)


def _tracker(P=None, hooks=False):
    from dvslam_amd import map_track as M
    P = P or lr.track_params()
    p = M.default_params(P.rows, P.cols, P.fx, P.fy, P.cx, P.cy, level_sigma2=P.level_sigma2, **{k: getattr(P, k) for k in mr.DEFAULTS if k != "n_levels"})
    return M.MapTracker(p, hooks=hooks)


def _dev(a):
    from dvslam_amd._lib import DeviceBuffer
    a = np.ascontiguousarray(a)
    return DeviceBuffer(max(a.nbytes, 64)).upload(a) if a.nbytes else DeviceBuffer(64)


def _check_selection(mb, what):
    """the dry getter against the restatement, bit for bit; the getter changes nothing -> (tables, geometry)"""
    T = _tables(mb)
    want = lr.geometry(*T)
    got = mb.landmark_geometry()
    assert got["best_obs_id"].tobytes() == want["best_obs_id"].tobytes(), what
    assert got["best_median"].tobytes() == want["best_median"].tobytes(), what
    assert got["n_counted"].tobytes() == want["n_counted"].tobytes(), what
    _same_tables(_tables(mb), T, (what, "dry getter"))
    return T, got


def _check_geometry(T, got, what):
    """within the forward bound of the longdouble restatement (tests/test_landmark_refresh_cpu.py has its derivation)"""
    ld = lr.geometry(*T, real=np.longdouble)
    worst = [0.0, 0.0]
    for s, m in enumerate(ld["n_counted"]):
        en = float(np.abs(got["normal"][s].astype(np.longdouble) - ld["normal"][s]).max())
        er = float((np.abs(got["range"][s].astype(np.longdouble) - ld["range"][s]) / np.maximum(np.abs(ld["range"][s]), np.longdouble(1e-300))).max())
        worst = [max(worst[0], en / lr.NORMAL_BOUND(int(m))), max(worst[1], er / lr.RANGE_BOUND)]
        assert en <= lr.NORMAL_BOUND(int(m)) and er <= lr.RANGE_BOUND, (what, s, int(m), en, er)
    print(what, "normal error / bound", worst[0], "range error / bound", worst[1])


def _refresh_both(mb, what, scope=None, **params):
    """the call on the handle and on the restatement of its own tables; only the landmark descriptor column may change"""
    T = _tables(mb)
    want, desc = lr.refresh(*T, scope_frame_id=scope, **params)
    got = mb.refresh_landmarks(scope, **params)
    assert got == want, (what, params, got, want)
    after = _tables(mb)
    _same_tables(after, T, what, but_desc=True)
    assert after[1]["desc"].tobytes() == desc.tobytes(), (what, params)
    return got, T, after


@pytest.fixture(scope="module")
def views_map(gpu):
    kfs, counts = lr.views_scene()
    mb = _handle(kfs)
    lr.leave_a_landmark_without_views(mb)
    yield mb, counts
    mb.close()


def test_views_scene_selection_min_views_scope_and_integrity(views_map):
    """one landmark each of 0, 1, 2, 3, 4, 7, 8, 9, 63, 64, 65, 255, 256, 257 and 300 views and 46 more: every path, lists longer than one
    wavefront and one workgroup take, identical descriptors and tied medians"""
    mb, counts = views_map
    T, geo = _check_selection(mb, "views scene")
    n = np.diff(T[1]["obs_offsets"])
    assert sorted(n.tolist()) == sorted(counts + [0]) and set(lr.VIEW_COUNTS + [0]) <= set(n.tolist())
    assert geo["best_median"][n == 0].tolist() == [-1] and geo["best_obs_id"][n == 0].tolist() == [int(lr.NO_VIEW_ID)]
    _check_geometry(T, geo, "views scene")
    # min_views on both sides of a count that exists: dry, so the map stays as it is for what follows
    for mv in (9, 10, 257, 258, 301):
        got, _, after = _refresh_both(mb, "min_views", min_views=mv, update_descriptors=0)
        assert after[1]["desc"].tobytes() == T[1]["desc"].tobytes() and got["max_views"] == 300 and got["n_without_views"] == 1
    dry = [mb.refresh_landmarks(min_views=mv, update_descriptors=0)["n_changed"] for mv in (9, 10, 257, 258, 301)]
    assert dry[0] > dry[1] > dry[2] == 1 and dry[3] == dry[4] == 0        # the landmarks of 9 views, and the one of 257, are in or out
    # keyframe scope: the whole-table result restricted to S_k, every other landmark's bytes untouched
    whole = lr.refresh(*T)[1]
    k = int(T[0]["frame_id"][8])
    got, _, after = _refresh_both(mb, "scope", scope=k)
    S = sorted(lr.scope_rows(*T, k))
    assert 0 < got["n_in_scope"] == len(S) < len(n) and got["n_changed"] > 0 and got["n_without_views"] == 0
    rest = np.setdiff1d(np.arange(len(n)), S)
    assert after[1]["desc"][S].tobytes() == whole[S].tobytes() and after[1]["desc"][rest].tobytes() == T[1]["desc"][rest].tobytes()
    # the whole table; a second refresh changes nothing; two identical dry getters give identical bytes
    got, _, after = _refresh_both(mb, "whole")
    assert got["n_in_scope"] == len(n) and got["n_changed"] > 0 and after[1]["desc"].tobytes() == whole.tobytes()
    again, _, _ = _refresh_both(mb, "second refresh")
    assert again["n_changed"] == 0
    a, b = mb.landmark_geometry(), mb.landmark_geometry()
    assert all(a[k].tobytes() == b[k].tobytes() for k in a)
    # the refreshed map goes on
    kf = dict(lr.views_scene()[0][5], frame_id=990000, stamp=(900, 0))
    res = lc.add(mb, kf)
    assert res["n_kept"] == len(kf["px"]) and res["n_associated"] == res["n_kept"]
    assert mb.covisibility(1)["weights"].shape == (301, 301)
    assert mb.cull_keyframes(apply=False)["n_keyframes"] == 301
    assert len(mb.window()["kf_frame_id"]) == 5
    mb.prune((2000, 0))
    _check_selection(mb, "after prune")


def test_hub_scene_landmark_seen_by_every_keyframe(gpu):
    mb = _handle(cr.hub_scene())
    T, geo = _check_selection(mb, "hub")
    n = np.diff(T[1]["obs_offsets"])
    assert n.max() == cr.HUB_NKF and geo["best_median"].max() == 0            # every view of a point carries one descriptor: all medians tie at 0
    _check_geometry(T, geo, "hub")
    got, _, _ = _refresh_both(mb, "hub")
    assert got["n_changed"] == 0 and got["max_views"] == cr.HUB_NKF
    got, _, _ = _refresh_both(mb, "hub scope", scope=cr.HUB_FRAME0 + cr.HUB_LEAF)
    assert got["n_in_scope"] == 4
    mb.close()


def test_fused_map_where_a_keyframe_names_a_landmark_twice(gpu):
    mb = _handle(br.make_scene())
    assert mb.fuse(cr.FUSED_QUERY, cr.FUSED_ENTRIES, **cr.FUSED_PARAMS)["n_fused"] > 0
    T, geo = _check_selection(mb, "fused")
    assert cr.repeated_pairs(*T) > 0
    _check_geometry(T, geo, "fused")
    got, _, _ = _refresh_both(mb, "fused scope", scope=cr.FUSED_QUERY)
    assert got["n_changed"] > 0
    got, _, _ = _refresh_both(mb, "fused")
    assert got["n_changed"] > 0
    assert _refresh_both(mb, "fused again")[0]["n_changed"] == 0
    mb.close()


def test_maps_of_none_one_and_two_keyframes_and_one_handle_through_sizes(gpu):
    from dvslam_amd import DvsError
    scene = br.make_scene()
    mb = _handle([])
    assert mb.refresh_landmarks() == dict(n_in_scope=0, n_changed=0, n_without_views=0, max_views=0)
    assert all(len(v) == 0 for v in mb.landmark_geometry().values())
    with pytest.raises(DvsError):
        mb.refresh_landmarks(12345)
    with pytest.raises(DvsError):
        mb.refresh_landmarks(min_views=0)
    for nk in (1, 2):
        lc.add(mb, scene[nk - 1])
        T, geo = _check_selection(mb, nk)
        _check_geometry(T, geo, nk)
        got, _, _ = _refresh_both(mb, nk)
        assert got["max_views"] == nk and got["n_in_scope"] == len(T[1]["id"])
    # small, big, small on one handle: the scratch only grows
    mb.reset()
    for kfs in (scene[:2], cr.hub_scene()[:40], scene[:3]):
        mb.reset()
        _handle(kfs, mb)
        T, geo = _check_selection(mb, len(kfs))
        _refresh_both(mb, len(kfs))
    mb.close()


def test_a_landmark_at_a_keyframe_centre_is_skipped(gpu):
    mb = _handle(br.make_scene()[:4])
    K, L, O = _tables(mb)
    s = int(np.argmax(np.diff(L["obs_offsets"])))
    views = lr.views(L, O)[s]
    f = int(O["frame_id"][views[0]])
    k = K["frame_id"].tolist().index(f)
    mb.apply_optimized({f: (K["R"][k], L["xyz"][s].astype(np.float64))}, {})        # the keyframe's centre becomes the landmark's position: r == 0
    T, geo = _check_selection(mb, "centre")
    assert geo["n_counted"][s] == len(views) - 1 and (geo["n_counted"] <= np.diff(T[1]["obs_offsets"])).all()
    _check_geometry(T, geo, "centre")
    mb.close()


# ---------------------------------------------------------------------------------------------------- the gates on host-made geometry
def _search_gated(mt, P, xyz, ldesc, kps, kdesc, normal, rg, cnt, R, t, **gates):
    """dvs_mapgate_search_device against the restatement: records, matches, counts and gate counts bit for bit -> (gate counts, result, records)"""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    bufs = [_dev(xyz), _dev(ldesc), _dev(kps), _dev(kdesc), _dev(np.ascontiguousarray(normal, np.float64)), _dev(np.ascontiguousarray(rg, np.float64)),
            _dev(np.ascontiguousarray(cnt, np.int32))]
    res = mt.search_gated(bufs[0], bufs[1], None, len(xyz), bufs[4], bufs[5], bufs[6], bufs[2], bufs[3], len(kps), R, t, **gates)
    rec = mt.landmark_records(); row, lid, dist, inl = mt.matches(); counts = mt.gate_counts()
    want, lm, d, wcounts = lr.search_gated(P, R, t, xyz, ldesc, kps, kdesc, normal, rg, cnt, **dict(lr.DEFAULT_GATES, **gates))
    for f in mr.LM_RECORD.names:
        assert rec[f].tobytes() == want[f].tobytes(), f
    assert (row == lm).all() and (dist == d).all() and not inl.any()
    assert counts.tolist() == wcounts.tolist()
    assert (res["status"], res["n_visible"], res["n_proposed"], res["n_matches"]) == (0, int(want["visible"].sum()), int(want["proposed"].sum()), int((lm >= 0).sum()))
    for b in bufs:
        b.free()
    return counts, res, rec


@pytest.fixture(scope="module")
def hook_tracker(gpu):
    mt = _tracker(mr.frame_params(), hooks=True)
    yield mt
    mt.close()


@pytest.mark.parametrize("n_lm", [63, 64, 65, 255, 256, 257])
def test_gated_search_equals_the_restatement(hook_tracker, n_lm):
    P = mr.frame_params()
    xyz, ld, kps, kd, normal, rg, cnt, R, t = lr.gate_scene(P, n_lm, 120, 100 + n_lm)
    counts, res, rec = _search_gated(hook_tracker, P, xyz, ld, kps, kd, normal, rg, cnt, R, t)
    assert (counts >= 10).all() and counts.sum() == sum(1 for j in range(n_lm) if j % 6 in (1, 2, 3, 4))     # each of the four tests is the one that fires
    assert rec["visible"][5::6].sum() > 0 and rec["visible"][0::6].sum() > 0 and not rec["visible"][1::6].any() and not rec["visible"][4::6].any()
    # other constants: gates wide open on distance, closed on the angle
    _search_gated(hook_tracker, P, xyz, ld, kps, kd, normal, rg, cnt, R, t, cos_min=0.0, range_factor=64.0)
    _search_gated(hook_tracker, P, xyz, ld, kps, kd, normal, rg, cnt, R, t, cos_min=1.0, range_factor=1.0)


def test_gates_at_exact_equality(hook_tracker):
    """lr.EXACT_GATE_CASES: X = (0, 0, 2) from O = 0, every quantity a small dyadic rational; a landmark passes at equality"""
    P = mr.frame_params()
    kps = mr.keypoints(np.array([[P.cx, P.cy]])); kd = np.zeros((1, 32), np.uint8)
    by_gates = {}
    for (N, dmin, dmax, m, cos_min, rf), want in lr.EXACT_GATE_CASES:
        by_gates.setdefault((cos_min, rf), []).append((N, dmin, dmax, m, want))
    for (cos_min, rf), cases in by_gates.items():
        n = len(cases)
        xyz = np.tile(np.array([0.0, 0.0, 2.0], np.float32), (n, 1)); ld = np.zeros((n, 32), np.uint8)
        normal = np.array([c[0] for c in cases]); rg = np.array([[c[1], c[2]] for c in cases]); cnt = np.array([c[3] for c in cases], np.int32)
        counts, res, rec = _search_gated(hook_tracker, P, xyz, ld, kps, kd, normal, rg, cnt, np.eye(3), np.zeros(3), cos_min=cos_min, range_factor=rf)
        assert rec["visible"].tolist() == [1 if c[4] < 0 else 0 for c in cases]
        assert counts.tolist() == [sum(1 for c in cases if c[4] == g) for g in range(4)]


def test_gates_that_exclude_nothing_give_the_ungated_bytes(hook_tracker):
    P = mr.frame_params()
    xyz, ld, kps, kd, normal, rg, cnt, R, t = lr.gate_scene(P, 257, 120, 357)
    mt = hook_tracker
    bufs = [_dev(xyz), _dev(ld), _dev(kps), _dev(kd), _dev(normal), _dev(rg), _dev(np.zeros(257, np.int32))]
    plain = mt.track_device(bufs[0], bufs[1], None, 257, bufs[2], bufs[3], len(kps), R, t)
    prec, pm = mt.landmark_records(), mt.matches()
    assert mt.gate_counts().tolist() == [0, 0, 0, 0]
    gated = mt.track_gated(bufs[0], bufs[1], None, 257, bufs[4], bufs[5], bufs[6], bufs[2], bufs[3], len(kps), R, t)      # m == 0 everywhere: every landmark passes
    grec, gm = mt.landmark_records(), mt.matches()
    assert mt.gate_counts().tolist() == [0, 0, 0, 0]
    assert all(np.asarray(plain[k]).tobytes() == np.asarray(gated[k]).tobytes() for k in plain)
    assert prec.tobytes() == grec.tobytes() and all(a.tobytes() == b.tobytes() for a, b in zip(pm, gm))
    assert plain["n_proposed"] > 50
    for b in bufs:
        b.free()


# ---------------------------------------------------------------------------------------------------- end to end
def _scipy_cost_ok(P, res, matches, xyz, kps):
    row, _, _, inl = matches
    ks = np.flatnonzero(row >= 0)
    X = np.array([[float(v) for v in xyz[j]] for j in row[ks]]); px = np.array([[float(kps[k]["x"]), float(kps[k]["y"])] for k in ks])
    Rcw, tcw = mr.pose_cw(res["R"], res["t"])
    opt = mr.scipy_optimum(P, Rcw, tcw, X, px, kps["octave"][ks], inl[ks])
    assert abs(res["cost"] - opt) <= 1e-6 * opt, (res["cost"], opt)


def test_drift_scene_matches_again_after_the_refresh(gpu):
    kfs, q = lr.drift_scene()
    P = lr.track_params()
    mb, mt = _handle(kfs), _tracker(P)
    T = _tables(mb)
    assert len(T[1]["id"]) == lr.DRIFT_N + lr.DRIFT_STATIC and (np.diff(T[1]["obs_offsets"]) == lr.DRIFT_NKF).all()
    d_kps, d_desc = _dev(q["kps"]), _dev(q["kdesc"])
    want0 = lr.matched_keypoints(P, q["R"], q["t"], T[1], q["kps"], q["kdesc"])
    r0 = mb.track_frame(mt, d_kps, d_desc, len(q["kps"]), q["R"], q["t"])
    row0 = mt.matches()[0]
    assert ((row0 >= 0) == want0).all() and not (row0 >= 0)[q["drifting"]].any() and r0["n_matches"] == lr.DRIFT_STATIC and r0["status"] == mr.OK
    got, _, after = _refresh_both(mb, "drift")
    assert got["n_changed"] == lr.DRIFT_N and got["max_views"] == lr.DRIFT_NKF
    want1 = lr.matched_keypoints(P, q["R"], q["t"], after[1], q["kps"], q["kdesc"])
    r1 = mb.track_frame(mt, d_kps, d_desc, len(q["kps"]), q["R"], q["t"])
    m1 = mt.matches()
    assert ((m1[0] >= 0) == want1).all() and (m1[0] >= 0).all() and r1["n_matches"] == lr.DRIFT_N + lr.DRIFT_STATIC and r1["status"] == mr.OK
    assert sorted(set(m1[2][q["drifting"]].tolist())) == [lr.DRIFT_QUERY_BITS - lr.DRIFT_STEP]
    _scipy_cost_ok(P, r1, m1, after[1]["xyz"], q["kps"])
    d_kps.free(); d_desc.free(); mt.close(); mb.close()


def test_wall_scene_gated_tracking_proposes_no_back_side_landmark(gpu):
    kfs, q = lr.wall_scene()
    P = lr.track_params()
    mb, mt = _handle(kfs), _tracker(P)
    T = _tables(mb)
    assert len(T[1]["id"]) == 2 * lr.WALL_N and (np.diff(T[1]["obs_offsets"]) == 3).all()
    geo = mb.landmark_geometry()
    back = geo["normal"][:, 2] < 0
    assert back.sum() == lr.WALL_N and (geo["n_counted"] == 3).all()
    g, wcounts = lr.gates(T[1]["xyz"], q["t"], geo["normal"], geo["range"], geo["n_counted"])
    assert ((g == lr.BACK) == back).all() and wcounts.tolist() == [0, 0, lr.WALL_N, 0]
    d_kps, d_desc = _dev(q["kps"]), _dev(q["kdesc"])
    before = _tables(mb)
    plain = mb.track_frame(mt, d_kps, d_desc, len(q["kps"]), q["R"], q["t"])
    pm = mt.matches()
    assert mt.gate_counts().tolist() == [0, 0, 0, 0]
    gated = mb.track_frame_gated(mt, d_kps, d_desc, len(q["kps"]), q["R"], q["t"])
    gm = mt.matches()
    assert mt.gate_counts().tolist() == wcounts.tolist()
    assert (plain["n_proposed"], gated["n_proposed"]) == (2 * lr.WALL_N, lr.WALL_N) and (plain["n_visible"], gated["n_visible"]) == (2 * lr.WALL_N, lr.WALL_N)
    assert plain["status"] == gated["status"] == mr.OK and gated["n_matches"] == lr.WALL_N
    assert not np.isin(gm[1][gm[0] >= 0], T[1]["id"][back].astype(np.int64)).any()
    _scipy_cost_ok(P, plain, pm, T[1]["xyz"], q["kps"])
    _scipy_cost_ok(P, gated, gm, T[1]["xyz"], q["kps"])
    # constants as wide as they go: only the back-facing test is left; and the map was never touched
    wide = mb.track_frame_gated(mt, d_kps, d_desc, len(q["kps"]), q["R"], q["t"], cos_min=0.0, range_factor=1e6)
    assert mt.gate_counts().tolist() == [0, 0, lr.WALL_N, 0]                     # back-facing does not depend on the constants
    assert wide["n_proposed"] == lr.WALL_N
    _same_tables(_tables(mb), before, "tracking")
    d_kps.free(); d_desc.free(); mt.close(); mb.close()
