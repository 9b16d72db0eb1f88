"""csrc/map_track.hip on the device against tests/map_track_ref.py.  Stages 1-3 on a 100 x 70 image (not a multiple of the 32-pixel
cell): every integer output and every stage-1 double bit for bit, over sizes around the wavefront and the workgroup and over hand-built
edge scenes.  Stage 4 on the CPU test's scene: the inlier flags exactly, the cost against the scipy optimum, identical bytes from identical
calls, and the three status paths."""
import ctypes as C
import numpy as np
import pytest
import map_track_ref as mr

pytestmark = pytest.mark.gpu

ROWS, COLS, F, CX, CY = 70, 100, 80.0, 50.0, 35.0
# z gates that are exact floats, so that a landmark can sit exactly on one
P0 = mr.Params(ROWS, COLS, F, F, CX, CY, min_z=0.5, max_z=4.0)
I3, Z3 = np.eye(3), np.zeros(3)


def _handle(P, hooks=True):
    from dvslam_amd import map_track as M
    p = M.default_params(P.rows, P.cols, P.fx, P.fy, P.cx, P.cy, level_sigma2=P.level_sigma2,
                         **{k: getattr(P, k) for k in mr.DEFAULTS if k != "n_levels"})
    return M.MapTracker(p, hooks=hooks)


@pytest.fixture(scope="module")
def trackers(gpu):
    made = {}

    def get(P):
        key = tuple(sorted((k, str(v)) for k, v in P.__dict__.items()))
        if key not in made:
            made[key] = _handle(P)
        return made[key]
    yield get
    for h in made.values():
        h.close()


def _dev(a):
    from dvslam_amd._lib import DeviceBuffer
    a = np.ascontiguousarray(a)
    return DeviceBuffer(max(a.nbytes, 64)).upload(a) if a.nbytes else DeviceBuffer(64)


def check_search(mt, P, xyz, ldesc, kps, kdesc, R=I3, t=Z3, ids=None):
    """the device's stages 1-3 against the reference, everything bit for bit -> the reference's (records, kp_lm, kp_dist)"""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3); ldesc = np.ascontiguousarray(ldesc, np.uint8).reshape(-1, 32)
    kdesc = np.ascontiguousarray(kdesc, np.uint8).reshape(-1, 32)
    bufs = [_dev(xyz), _dev(ldesc), _dev(ids) if ids is not None else None, _dev(kps), _dev(kdesc)]
    res = mt.search_device(bufs[0], bufs[1], bufs[2], len(xyz), bufs[3], bufs[4], len(kps), R, t)
    rec = mt.landmark_records(); start, order = mt.cells(); row, lid, dist, inl = mt.matches()
    Rcw, tcw = mr.pose_cw(R, t)
    want = mr.search_grid(P, Rcw, tcw, xyz, ldesc, kps, kdesc)
    lm, d = mr.assign(want, len(kps))
    wstart, worder, unb = mr.bin_keypoints(P, kps)
    assert (start == wstart).all() and (order == worder).all()
    for f in mr.LM_RECORD.names:
        assert rec[f].tobytes() == want[f].tobytes(), f
    assert (row == lm).all() and (dist == d).all() and not inl.any()
    all_ids = np.arange(len(xyz), dtype=np.int64) if ids is None else np.asarray(ids, np.int64)
    want_id = np.array([all_ids[j] if j >= 0 else -1 for j in lm], np.int64)
    assert (lid == want_id).all()
    assert (res["status"], res["n_visible"], res["n_proposed"], res["n_matches"], res["n_unbinned"], res["n_inliers"]) == \
        (0, int(want["visible"].sum()), int(want["proposed"].sum()), int((lm >= 0).sum()), unb, 0)
    assert res["R"].tobytes() == np.asarray(R, np.float64).tobytes() and res["t"].tobytes() == np.asarray(t, np.float64).tobytes() and res["cost"] == 0.0
    for b in bufs:
        if b is not None:
            b.free()
    return want, lm, d


# ---------------------------------------------------------------------------------------------------- sizes
@pytest.mark.parametrize("n_lm", [0, 1, 63, 64, 65, 257])
def test_landmark_counts_around_a_wavefront_and_a_workgroup(trackers, n_lm):
    R, t = mr.rot("y", 3.0) @ mr.rot("x", -2.0), np.array([0.05, -0.02, 0.1])
    xyz, ld, kps, kd = mr.search_scene(P0, n_lm, 150, 20 + n_lm, R, t)
    ids = np.cumsum(np.random.default_rng(n_lm).integers(1, 9, n_lm)).astype(np.int64) + (1 << 40)
    want, lm, _ = check_search(trackers(P0), P0, xyz, ld, kps, kd, R, t, ids if n_lm else None)
    if n_lm >= 63:
        assert want["visible"].sum() > n_lm // 2 and 0 < (lm >= 0).sum() <= want["proposed"].sum()
    if n_lm == 257:
        assert (lm >= 0).sum() < want["proposed"].sum() and (want["d_second"] >= 0).sum() > 100


@pytest.mark.parametrize("n_kp", [0, 1, 70])
def test_keypoint_counts_none_one_and_seventy_in_one_cell(trackers, n_kp):
    xyz, ld, kps, kd = mr.search_scene(P0, 65, n_kp, 40 + n_kp)
    if n_kp == 70:                                   # more than a wavefront's worth in cell (1, 1); the landmarks come along
        rng = np.random.default_rng(1)
        kps["x"] = (32 + rng.uniform(0, 31.9, 70)).astype(np.float32); kps["y"] = (32 + rng.uniform(0, 31.9, 70)).astype(np.float32)
        z = xyz[:, 2].astype(np.float64)
        xyz[:, 0] = ((kps["x"][np.arange(65) % 70] + 1.5 - CX) * z / F).astype(np.float32)
        xyz[:, 1] = ((kps["y"][np.arange(65) % 70] - 1.0 - CY) * z / F).astype(np.float32)
    want, lm, _ = check_search(trackers(P0), P0, xyz, ld, kps, kd)
    if n_kp == 70:
        start, _, _ = mr.bin_keypoints(P0, kps)
        assert start[1 * 4 + 1 + 1] - start[1 * 4 + 1] == 70 and (want["d_second"] >= 0).sum() > 50 and (lm >= 0).sum() > 10


@pytest.mark.parametrize("cell", [8, 1000])
def test_outcome_does_not_depend_on_the_cell_size(trackers, cell):
    xyz, ld, kps, kd = mr.search_scene(P0, 257, 150, 3)
    a, lm_a, d_a = check_search(trackers(P0), P0, xyz, ld, kps, kd)
    Pc = P0.with_(cell=cell)
    b, lm_b, d_b = check_search(trackers(Pc), Pc, xyz, ld, kps, kd)
    assert a.tobytes() == b.tobytes() and (lm_a == lm_b).all() and (d_a == d_b).all()


def test_radius_larger_than_the_image(trackers):
    Pr = P0.with_(radius=500.0)
    xyz, ld, kps, kd = mr.search_scene(Pr, 65, 40, 8)
    want, lm, _ = check_search(trackers(Pr), Pr, xyz, ld, kps, kd)
    assert (want["d_second"][want["visible"] == 1] >= 0).all()           # every keypoint is a candidate of every visible landmark


# ---------------------------------------------------------------------------------------------------- hand-built edges (identity pose)
def lm_at(u, v, z=1.0):
    return [(u - CX) * z / F, (v - CY) * z / F, z]


def bits(n):
    """a descriptor with the first n bits set: its distance to the zero descriptor is n"""
    d = np.zeros(32, np.uint8)
    for b in range(n):
        d[b >> 3] |= np.uint8(1 << (b & 7))
    return d


def scene(lms, kps_xy_bits, octave=0):
    xyz = np.array(lms, np.float32).reshape(-1, 3)
    kps = mr.keypoints([(x, y) for x, y, _ in kps_xy_bits], octave)
    kd = np.array([bits(b) for _, _, b in kps_xy_bits], np.uint8).reshape(-1, 32)
    return xyz, np.zeros((len(xyz), 32), np.uint8), kps, kd


NEXT = lambda x: float(np.nextafter(np.float32(x), np.float32(np.inf)))    # noqa: E731
PREV = lambda x: float(np.nextafter(np.float32(x), np.float32(-np.inf)))   # noqa: E731


def test_keypoint_exactly_on_the_window_edge_and_just_outside(trackers):
    # landmark 0 at (50, 35): keypoint 0 at dx == radius is kept although keypoint 1, one float further out, would be nearer in Hamming;
    # landmark 1 at (30, 15): keypoint 2 at dy == -radius is kept, keypoint 3 has dx just over the radius
    xyz, ld, kps, kd = scene([lm_at(50, 35), lm_at(30, 15)], [(65.0, 35.0, 5), (NEXT(65.0), 35.0, 0), (30.0, 0.0, 7), (NEXT(45.0), 15.0, 0)])
    want, lm, d = check_search(trackers(P0), P0, xyz, ld, kps, kd)
    assert want["u"].tolist() == [50.0, 30.0] and want["v"].tolist() == [35.0, 15.0]
    assert want["best_k"].tolist() == [0, 2] and want["d_best"].tolist() == [5, 7] and want["d_second"].tolist() == [-1, -1]
    assert lm.tolist() == [0, -1, 1, -1]


def test_projections_on_the_image_border(trackers):
    # u == 0 and v == 0 are visible, u == cols and v == rows are not
    xyz, ld, kps, kd = scene([lm_at(0, 35), lm_at(100, 35), lm_at(50, 0), lm_at(50, 70), lm_at(PREV(100.0), 35)],
                             [(0.0, 35.0, 1), (99.5, 35.0, 2), (50.0, 0.0, 3), (50.0, 69.5, 4)])
    want, lm, _ = check_search(trackers(P0), P0, xyz, ld, kps, kd)
    assert want["visible"].tolist() == [1, 0, 1, 0, 1]
    assert want["u"][0] == 0.0 and want["v"][2] == 0.0 and want["u"][1] == 0.0 and want["best_k"].tolist() == [0, -1, 2, -1, 1]


def test_depth_exactly_at_each_gate_and_behind_the_camera(trackers):
    zs = [0.5, NEXT(0.5), 4.0, PREV(4.0), -1.0, 0.0]
    xyz, ld, kps, kd = scene([lm_at(50, 35, z) for z in zs], [(50.0, 35.0, 1)])
    want, lm, _ = check_search(trackers(P0), P0, xyz, ld, kps, kd)
    assert want["visible"].tolist() == [0, 1, 0, 1, 0, 0] and lm.tolist() == [1]   # rows 1 and 3 tie at distance 1: the lower row keeps it
    assert want["kept"].tolist() == [0, 1, 0, 0, 0, 0] and want["proposed"].tolist() == [0, 1, 0, 1, 0, 0]


def test_window_over_four_cells_and_the_last_partial_cells(trackers):
    # landmark 0 at (32, 32): its window [17, 47]^2 meets cells (0,0) (1,0) (0,1) (1,1); the nearest descriptor sits in the last of them.
    # landmark 1 at (97, 67): cells (2..3, 1..2), the match in the partial cell (3, 2) of 4 x 6 pixels
    xyz, ld, kps, kd = scene([lm_at(32, 32), lm_at(97, 67)],
                             [(20.0, 20.0, 30), (40.0, 20.0, 20), (20.0, 40.0, 25), (40.0, 40.0, 3), (16.5, 32.0, 0), (99.5, 69.5, 2), (83.0, 53.0, 30),
                              (81.5, 60.0, 0)])
    want, lm, _ = check_search(trackers(P0), P0, xyz, ld, kps, kd)
    assert want["best_k"].tolist() == [3, 5] and want["d_second"].tolist() == [20, 30] and lm.tolist() == [-1, -1, -1, 0, -1, 1, -1, -1]


def test_equal_distances_lowest_keypoint_wins_and_the_ratio_rejects(trackers):
    xyz, ld, kps, kd = scene([lm_at(50, 35)], [(55.0, 35.0, 9), (45.0, 35.0, 4), (50.0, 40.0, 4), (50.0, 30.0, 4)])
    want, lm, _ = check_search(trackers(P0), P0, xyz, ld, kps, kd)
    assert (want["best_k"][0], want["d_best"][0], want["d_second"][0], want["proposed"][0]) == (1, 4, 4, 0) and (lm == -1).all()
    Pn = P0.with_(ratio_pct=0)
    want, lm, _ = check_search(trackers(Pn), Pn, xyz, ld, kps, kd)
    assert want["proposed"][0] == 1 and lm.tolist() == [-1, 0, -1, -1]


def test_two_landmarks_tie_on_one_keypoint_lower_id_wins_loser_unmatched(trackers):
    # both see keypoint 0 at distance 5 and keypoint 1 at distance 40; row 0 keeps keypoint 0, row 1 gets nothing although keypoint 1 is free
    xyz, ld, kps, kd = scene([lm_at(50, 35), lm_at(52, 35)], [(51.0, 35.0, 5), (51.0, 40.0, 40)])
    ids = np.array([10, 20], np.int64)
    want, lm, d = check_search(trackers(P0), P0, xyz, ld, kps, kd, ids=ids)
    assert want["proposed"].tolist() == [1, 1] and want["kept"].tolist() == [1, 0] and lm.tolist() == [0, -1] and d.tolist() == [5, -1]


def test_distance_equal_to_max_hamming_is_rejected(trackers):
    xyz, ld, kps, kd = scene([lm_at(30, 35), lm_at(70, 35)], [(30.0, 35.0, 50), (70.0, 35.0, 49)])
    want, lm, _ = check_search(trackers(P0), P0, xyz, ld, kps, kd)
    assert want["d_best"].tolist() == [50, 49] and want["proposed"].tolist() == [0, 1] and lm.tolist() == [-1, 1]


def test_ratio_test_at_equality_and_switched_off(trackers):
    # 9 * 100 == 90 * 10: rejected; 8 * 100 < 90 * 10: accepted
    xyz, ld, kps, kd = scene([lm_at(30, 35), lm_at(70, 35)], [(30.0, 35.0, 9), (31.0, 35.0, 10), (70.0, 35.0, 8), (71.0, 35.0, 10)])
    want, lm, _ = check_search(trackers(P0), P0, xyz, ld, kps, kd)
    assert want["proposed"].tolist() == [0, 1] and lm.tolist() == [-1, -1, 1, -1]
    Pn = P0.with_(ratio_pct=0)
    want, lm, _ = check_search(trackers(Pn), Pn, xyz, ld, kps, kd)
    assert want["proposed"].tolist() == [1, 1] and lm.tolist() == [0, -1, 1, -1]


def test_unbinned_keypoints_in_the_device_form_and_refused_in_the_host_form(trackers):
    xyz, ld, kps, kd = scene([lm_at(50, 35)], [(50.0, 35.0, 0)] * 6 + [(51.0, 35.0, 6)])
    kps["x"][0] = -1.0; kps["x"][1] = 100.0; kps["y"][2] = 70.0; kps["x"][3] = np.nan; kps["octave"][4] = 8; kps["octave"][5] = -1
    mt = trackers(P0)
    want, lm, _ = check_search(mt, P0, xyz, ld, kps, kd)
    assert want["best_k"][0] == 6 and want["d_second"][0] == -1 and lm.tolist() == [-1] * 6 + [0]
    from dvslam_amd._lib import DvsError
    for k in range(6):
        with pytest.raises(DvsError) as e:
            mt.track(xyz, ld, None, kps[[k, 6]], kd[[k, 6]], I3, Z3)
        assert e.value.code == -6
    r = mt.track(xyz, ld, None, kps[6:], kd[6:], I3, Z3)
    assert (r["status"], r["n_matches"], r["n_unbinned"]) == (mr.FEW_MATCHES, 1, 0)
    with pytest.raises(DvsError) as e:
        mt.track(np.repeat(xyz, 2, 0), np.repeat(ld, 2, 0), np.array([5, 5], np.int64), kps[6:], kd[6:], I3, Z3)
    assert e.value.code == -6
    with pytest.raises(DvsError) as e:
        mt.track(xyz, ld, None, kps[6:], kd[6:], I3, np.array([0.0, np.nan, 0.0]))
    assert e.value.code == -6


# ---------------------------------------------------------------------------------------------------- stage 4
@pytest.fixture(scope="module")
def noisy():
    """the CPU test's scene and the reference's result; asserted here, on the CPU: no chi lies within 1e-6 relative of the gate at any of
    the four classifications (the nearest is some 4e-2 away), so rounding in sin / cos cannot decide a flag"""
    s = mr.refine_scene()
    r = mr.refine(s["P"], s["R0"], s["t0"], s["X"], s["px"], s["oct"])
    assert r["status"] == mr.OK and len(r["chi_rounds"]) == 4 and mr.gate_margin(s["P"], r) > 1e-6
    return s, r


def _refine(mt, s, n=None):
    X, px, oc = s["X"][:n], s["px"][:n], s["oct"][:n]
    bufs = [_dev(X), _dev(px), _dev(oc.astype(np.int32))]
    res = mt.refine_device(bufs[0], bufs[1], bufs[2], len(X), s["R0"], s["t0"])
    m = mt.matches()
    for b in bufs:
        b.free()
    return res, m


def test_refinement_flags_cost_and_determinism(trackers, noisy):
    s, want = noisy
    mt = trackers(s["P"])
    res, (row, lid, dist, inl) = _refine(mt, s)
    print("cost", res["cost"], "reference", want["cost"], "inliers", res["n_inliers"], want["n_inliers"])
    assert res["status"] == mr.OK and res["n_matches"] == 300
    assert (inl == want["inlier"]).all() and res["n_inliers"] == want["n_inliers"]
    assert (row == np.arange(300)).all() and (lid == np.arange(300)).all() and not dist.any()
    opt = mr.scipy_optimum(s["P"], want["Rcw"], want["tcw"], s["X"], s["px"], s["oct"], want["inlier"])
    assert abs(res["cost"] - opt) <= 1e-6 * opt, (res["cost"], opt)
    assert np.abs(res["R"] - want["R"]).max() < 1e-9 and np.abs(res["t"] - want["t"]).max() < 1e-9
    res2, m2 = _refine(mt, s)
    for k in ("R", "t"):
        assert res[k].tobytes() == res2[k].tobytes()
    assert np.float64(res["cost"]).tobytes() == np.float64(res2["cost"]).tobytes() and (m2[3] == inl).all()
    assert {k: res[k] for k in ("status", "n_matches", "n_inliers")} == {k: res2[k] for k in ("status", "n_matches", "n_inliers")}


def test_whole_frame_host_form_equals_the_reference(trackers):
    s = mr.track_scene()
    want = mr.track(s["P"], s["R0"], s["t0"], s["xyz"], s["ldesc"], s["kps"], s["kdesc"])
    assert want["status"] == mr.OK and mr.gate_margin(s["P"], want) > 1e-6 and want["n_matches"] > 250 and (want["inlier"] == 0).sum() > 20
    mt = trackers(s["P"])
    res = mt.track(s["xyz"], s["ldesc"], s["ids"], s["kps"], s["kdesc"], s["R0"], s["t0"])
    row, lid, dist, inl = mt.matches()
    rec = mt.landmark_records()
    for f in mr.LM_RECORD.names:
        assert rec[f].tobytes() == want["rec"][f].tobytes(), f
    assert (row == want["kp_lm"]).all() and (dist == want["kp_dist"]).all() and (inl == want["kp_inlier"]).all()
    assert (lid == np.where(row >= 0, s["ids"][np.maximum(row, 0)], -1)).all()
    assert {k: res[k] for k in ("status", "n_visible", "n_proposed", "n_matches", "n_inliers", "n_unbinned")} == \
        {k: want[k] for k in ("status", "n_visible", "n_proposed", "n_matches", "n_inliers", "n_unbinned")}
    assert abs(res["cost"] - want["cost"]) <= 1e-9 * want["cost"]
    assert np.abs(res["R"] - want["R"]).max() < 1e-10 and np.abs(res["t"] - want["t"]).max() < 1e-10
    assert np.abs(res["t"] - s["t_true"]).max() < np.abs(s["t0"] - s["t_true"]).max()
    res2 = mt.track(s["xyz"], s["ldesc"], s["ids"], s["kps"], s["kdesc"], s["R0"], s["t0"])
    assert all(np.asarray(res[k]).tobytes() == np.asarray(res2[k]).tobytes() for k in res)


def test_fourteen_pairs_are_too_few(trackers, noisy):
    s, _ = noisy
    mt = trackers(s["P"])
    res, (_, _, _, inl) = _refine(mt, s, 14)
    assert (res["status"], res["n_matches"], res["n_inliers"], res["cost"]) == (mr.FEW_MATCHES, 14, 0, 0.0) and not inl.any()
    assert res["R"].tobytes() == np.ascontiguousarray(s["R0"]).tobytes() and res["t"].tobytes() == s["t0"].tobytes()
    t = mr.track_scene()                             # ... and fourteen kept pairs through the search: fourteen of the frame's keypoints
    want = mr.track(t["P"], t["R0"], t["t0"], t["xyz"], t["ldesc"], t["kps"][:14], t["kdesc"][:14])
    assert (want["status"], want["n_matches"]) == (mr.FEW_MATCHES, 14)
    r = mt.track(t["xyz"], t["ldesc"], t["ids"], t["kps"][:14], t["kdesc"][:14], t["R0"], t["t0"])
    assert (r["status"], r["n_matches"], r["n_inliers"]) == (mr.FEW_MATCHES, 14, 0) and r["R"].tobytes() == np.ascontiguousarray(t["R0"]).tobytes()
    assert (mt.matches()[0] == want["kp_lm"]).all() and not mt.matches()[3].any()
    res, _ = _refine(mt, s, 15)
    assert res["status"] != mr.FEW_MATCHES


def test_three_pairs_with_one_point_are_degenerate(trackers, noisy):
    s, _ = noisy
    P3 = s["P"].with_(min_matches=3)
    d = dict(s, X=np.repeat(s["X"][:1], 3, 0), px=np.repeat(s["px"][:1], 3, 0), oct=s["oct"][:3] * 0)
    assert mr.refine(P3, d["R0"], d["t0"], d["X"], d["px"], d["oct"])["status"] == mr.DEGENERATE
    res, (_, _, _, inl) = _refine(trackers(P3), d)
    assert (res["status"], res["n_matches"], res["n_inliers"], res["cost"]) == (mr.DEGENERATE, 3, 0, 0.0) and not inl.any()
    assert res["R"].tobytes() == np.ascontiguousarray(s["R0"]).tobytes() and res["t"].tobytes() == s["t0"].tobytes()


def test_gross_outliers_only_leave_too_few_inliers(trackers):
    g = mr.outlier_scene()
    want = mr.refine(g["P"], g["R0"], g["t0"], g["X"], g["px"], g["oct"])
    assert want["status"] == mr.FEW_INLIERS and mr.gate_margin(g["P"], want) > 1e-6
    res, (_, _, _, inl) = _refine(trackers(g["P"]), g)
    print("inliers", res["n_inliers"], "reference", want["n_inliers"])
    assert res["status"] == mr.FEW_INLIERS and res["n_inliers"] < g["P"].min_inliers
    assert res["R"].tobytes() == np.ascontiguousarray(g["R0"]).tobytes() and res["t"].tobytes() == g["t0"].tobytes()
    assert (inl == want["inlier"]).all()
