"""Tracking against the map through the handles that own the data: dvs_backend_track_frame over the backend's landmark table as it stands
(the map read back through the getters is what the reference runs on, and it must not change), and dvs_tracker_track_map over the
tracker's last depth-filtered features — as a dry run, which must leave the tracker as it was, and applied, after which the next frame's
odometry composes on the refined pose."""
import numpy as np
import pytest
import backend_ref as br
import map_track_ref as mr

pytestmark = pytest.mark.gpu


def _map_tracker(rows, cols, fx, fy, cx, cy, **kw):
    from dvslam_amd import map_track as M
    return M.MapTracker(M.default_params(rows, cols, fx, fy, cx, cy, **kw), hooks=True)


def _same_tables(a, b):
    for x, y in zip(a, b):
        assert set(x) == set(y)
        for k in x:
            assert np.asarray(x[k]).tobytes() == np.asarray(y[k]).tobytes(), k


def _compare(res, mt, want, ids):
    row, lid, dist, inl = mt.matches()
    rec = mt.landmark_records()
    for f in mr.LM_RECORD.names:
        assert rec[f].tobytes() == want["rec"][f].tobytes(), f
    assert (row == want["kp_lm"]).all() and (dist == want["kp_dist"]).all() and (inl == want["kp_inlier"]).all()
    assert (lid == np.array([int(ids[j]) if j >= 0 else -1 for j in row], np.int64)).all()
    keys = ("status", "n_visible", "n_proposed", "n_matches", "n_inliers", "n_unbinned")
    assert {k: res[k] for k in keys} == {k: want[k] for k in keys}
    if want["status"] == mr.OK:
        assert abs(res["cost"] - want["cost"]) <= 1e-9 * want["cost"]
        assert np.abs(res["R"] - want["R"]).max() < 1e-10 and np.abs(res["t"] - want["t"]).max() < 1e-10
    else:
        assert res["R"].tobytes() == np.ascontiguousarray(want["R"]).tobytes() and res["t"].tobytes() == want["t"].tobytes()


def test_backend_track_frame_equals_the_reference_on_the_getters_arrays(gpu):
    from dvslam_amd.backend import MappingBackend
    from dvslam_amd._lib import DeviceBuffer
    rng = np.random.default_rng(5)
    n = 60
    X = np.stack([rng.uniform(-1.2, 1.2, n), rng.uniform(-0.9, 0.9, n), rng.uniform(2.5, 4.5, n)], 1)
    D = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    Rz = np.diag([-1.0, -1.0, 1.0])                                       # br.Q_Z180 as a matrix

    def view(t):
        c = (X - t) @ Rz                                                  # R^T (X - t), R symmetric
        return np.stack([br.FX * c[:, 0] / c[:, 2] + br.CX, br.FY * c[:, 1] / c[:, 2] + br.CY], 1)
    mb = MappingBackend(br.FX, br.FY, br.CX, br.CY, filtered=("person",), initial_capacity=64)
    for k in range(2):
        t = np.array([0.3 * k, 0.0, 0.0])
        mb.add_keyframe(k, (k, 0), t, br.Q_Z180, X + rng.normal(0, 0.01, (n, 3)), view(t) + rng.normal(0, 0.2, (n, 2)), D.copy())
    before = (mb.landmarks(), mb.observations(), mb.keyframes())
    lm = before[0]
    assert 55 <= len(lm["id"]) <= 70 and (np.diff(lm["id"].astype(np.int64)) > 0).all()
    # a third view between the two, its keypoints in another order, a few bits of every descriptor flipped, the prior a little off
    t_true = np.array([0.14, 0.03, -0.02])
    perm = rng.permutation(n)
    kps = mr.keypoints((view(t_true) + rng.normal(0, 0.3, (n, 2)))[perm].astype(np.float32))
    kps["octave"] = rng.integers(0, 3, n)
    kd = D[perm].copy()
    for k in range(n):
        for b in rng.choice(256, 5, replace=False):
            kd[k, b >> 3] ^= np.uint8(1 << (b & 7))
    R0, t0 = Rz @ mr.rot("y", 0.4) @ mr.rot("x", -0.3), t_true + np.array([0.01, -0.008, 0.012])
    P = mr.Params(480, 640, br.FX, br.FY, br.CX, br.CY)
    want = mr.track(P, R0, t0, lm["xyz"], lm["desc"], kps, kd)
    assert want["status"] == mr.OK and want["n_matches"] >= 40 and mr.gate_margin(P, want) > 1e-6
    mt = _map_tracker(480, 640, br.FX, br.FY, br.CX, br.CY)
    d_k, d_d = DeviceBuffer(kps.nbytes).upload(kps), DeviceBuffer(kd.nbytes).upload(kd)
    res = mb.track_frame(mt, d_k, d_d, n, R0, t0)
    _compare(res, mt, want, lm["id"])
    assert res["n_inliers"] >= 40 and np.abs(res["t"] - t_true).max() < 0.03      # (the map itself carries a centimetre of noise)
    _same_tables(before, (mb.landmarks(), mb.observations(), mb.keyframes()))
    # an empty map: nothing to match, the prior comes back
    mb.reset()
    res = mb.track_frame(mt, d_k, d_d, n, R0, t0)
    assert (res["status"], res["n_matches"], res["n_visible"]) == (mr.FEW_MATCHES, 0, 0) and res["R"].tobytes() == np.ascontiguousarray(R0).tobytes()
    d_k.free(); d_d.free(); mt.close(); mb.close()


COLS, ROWS, F = 640, 480, 600.0


def _run(tr, frames, depth, mb=None, mt=None, apply_at=None, apply=False):
    """the frames through the tracker; keyframes go to `mb` when it is given; after frame `apply_at` one dvs_tracker_track_map"""
    out, tm = [], None
    for i, f in enumerate(frames):
        r, payload = tr.track(f, depth, (i, 0))
        if mb is not None and payload is not None and (apply_at is None or i < apply_at):
            mb.add_keyframe_cdr(payload)
        out.append(r)
        if i == apply_at:
            tm = tr.track_map(mb, mt, apply=apply)
    return out, tm


def test_tracker_track_map_dry_run_and_applied(gpu):
    from dvslam_amd import synth, tracker as T
    from dvslam_amd.backend import MappingBackend
    frames = [synth.make_traj_frame(t, COLS, ROWS, seed=1234) for t in range(4)]
    depth = np.full((ROWS, COLS), 1500, np.uint16)
    tr = T.Tracker(T.default_params(ROWS, COLS, F, F, COLS / 2.0, ROWS / 2.0, nfeatures=500))
    mb = MappingBackend(F, F, COLS / 2.0, ROWS / 2.0, filtered=())
    mt = _map_tracker(ROWS, COLS, F, F, COLS / 2.0, ROWS / 2.0)
    plain, _ = _run(tr, frames, depth)                                     # no map tracking at all
    tr.reset()
    dry, res = _run(tr, frames, depth, mb, mt, apply_at=2, apply=False)
    assert mb.counts()["n_keyframes"] == 2 and mb.counts()["n_landmarks"] > 100
    for a, b in zip(plain, dry):                                          # the dry run changed nothing, the frame after it included
        assert set(a) == set(b) and all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a)
    # the reference over what the getters return: the features of frame 2 are gone from the tracker by now, so run to frame 2 again
    tr.reset()
    upto2, _ = _run(tr, frames[:3], depth)
    kps, kd = tr.filtered_features()
    assert len(kps) == upto2[2]["n_filtered"] > 100
    lm = mb.landmarks()
    P = mr.Params(ROWS, COLS, F, F, COLS / 2.0, ROWS / 2.0)
    want = mr.track(P, upto2[2]["R"], upto2[2]["t"], lm["xyz"], lm["desc"], kps, kd)
    print("status", want["status"], "matches", want["n_matches"], "inliers", want["n_inliers"], "margin", mr.gate_margin(P, want))
    assert mr.gate_margin(P, want) > 1e-6
    again = tr.track_map(mb, mt, apply=False)
    _compare(again, mt, want, lm["id"])
    assert all(np.asarray(again[k]).tobytes() == np.asarray(res[k]).tobytes() for k in res)      # the same call twice: the same bytes
    assert want["status"] == mr.OK
    # applied: the tracker's pose is the refined one, and frame 3 composes its motion on it
    refined = tr.track_map(mb, mt, apply=True)
    assert all(np.asarray(refined[k]).tobytes() == np.asarray(res[k]).tobytes() for k in res)
    r3, _ = tr.track(frames[3], depth, (3, 0))
    assert r3["pose_updated"] == 1 and plain[3]["pose_updated"] == 1
    assert r3["rvec"].tobytes() == plain[3]["rvec"].tobytes() and r3["tvec"].tobytes() == plain[3]["tvec"].tobytes()   # the odometry itself is the same
    Ri = plain[2]["R"].T @ plain[3]["R"]; ti = plain[2]["R"].T @ (plain[3]["t"] - plain[2]["t"])                        # frame 3's motion
    assert np.abs(r3["R"] - refined["R"] @ Ri).max() < 1e-12 and np.abs(r3["t"] - (refined["t"] + refined["R"] @ ti)).max() < 1e-12
    assert r3["R"].tobytes() != plain[3]["R"].tobytes()
    tr.close(); mt.close(); mb.close()
