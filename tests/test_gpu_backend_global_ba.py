"""GPU: dvs_backend_global_ba / MappingBackend.global_bundle_adjust — global BA of the map the backend keeps on the device — against the
restated assembly rule (tests/global_ba_ref.py) and the same problem solved directly through BAProblem.solve_global."""
import functools
import numpy as np
import pytest
import backend_ref as br
import global_ba_ref as gr
import loop_closing_ref as lc

pytestmark = pytest.mark.gpu
FX, FY, CX, CY = 500.0, 500.0, 320.0, 240.0
NKF, RADIUS, DTHETA = 70, 20.0, 0.02


def _Ry(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


def _quat_xyzw(R):
    w = np.sqrt(max(0.0, 1 + R[0, 0] + R[1, 1] + R[2, 2])) / 2            # small rotations only: w is far from 0
    return np.array([(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w])


@functools.lru_cache(maxsize=None)
def arc_keyframes(seed=11):
    """70 keyframes on an arc of radius 20 m looking outward, 0.4 m apart, so a point 3 m out crosses the image in about 8 keyframes;
    about 48 observations per keyframe; the reported poses drift smoothly (up to 4 cm and 0.5 degrees at the end); pixels carry 0.5 px
    noise; the reported landmark positions are the true camera-frame points seen through the reported pose; no detections."""
    rng = np.random.default_rng(seed)
    th0, th1 = -0.12, (NKF - 1) * DTHETA + 0.12
    npts = 560
    phi = rng.uniform(th0, th1, npts); rad = RADIUS + rng.uniform(2.6, 3.4, npts)
    X = np.stack([rad * np.sin(phi), rng.uniform(-0.9, 0.9, npts), rad * np.cos(phi) - RADIUS], 1)
    D = rng.integers(0, 256, (npts, 32), dtype=np.uint8)
    out = []
    for k in range(NKF):
        th = k * DTHETA
        R = _Ry(th); C = np.array([RADIUS * np.sin(th), 0.0, RADIUS * np.cos(th) - RADIUS])
        xc = (X - C) @ R                                                    # R^T (X - C)
        u = FX * xc[:, 0] / xc[:, 2] + CX; v = FY * xc[:, 1] / xc[:, 2] + CY
        vis = np.nonzero((xc[:, 2] > 0.5) & (u > 8) & (u < 632) & (v > 8) & (v < 472))[0]
        vis = vis[rng.permutation(len(vis))]
        px = np.stack([u[vis], v[vis]], 1) + rng.normal(0, 0.5, (len(vis), 2))
        desc = D[vis].copy()
        for r in range(len(vis)):
            for b in rng.choice(256, rng.integers(0, 6), replace=False):
                desc[r, b >> 3] ^= np.uint8(1 << (b & 7))
        f = k / (NKF - 1)
        Rr = R @ _Ry(np.deg2rad(0.5) * f * f); tr = C + np.array([0.04, 0.01, -0.03]) * f * f
        out.append(dict(frame_id=500 + k, stamp=(100 + k, 0), t=tr, q=_quat_xyzw(Rr), xyz=xc[vis] @ Rr.T + tr, px=px, desc=desc, det=[]))
    return out


def _arc_handle():
    from dvslam_amd.backend import MappingBackend
    mb = MappingBackend(FX, FY, CX, CY, filtered=(), initial_capacity=64)
    for kf in arc_keyframes():
        lc.add(mb, kf)
    return mb


def _tables(mb):
    return mb.landmarks(), mb.observations(), mb.keyframes()


def _same_bytes(a, b):
    for x, y in zip(a, b):
        assert set(x) == set(y)
        for k in x:
            assert np.asarray(x[k]).tobytes() == np.asarray(y[k]).tobytes(), k


def test_global_ba_of_a_70_keyframe_map(gpu):
    """fails without the feature (no global_bundle_adjust).  The assembled problem is the restatement's; a run that does not converge
    leaves every byte of the map; a converged run leaves exactly the parameters of the same problem solved directly."""
    from dvslam_amd import BAProblem
    mb = _arc_handle()
    before = _tables(mb)
    lms, obs, kfs = before
    per_kf = np.bincount([int(f) - 500 for f in obs["frame_id"]], minlength=NKF)
    assert len(kfs["frame_id"]) == NKF and 35 <= per_kf.min() and per_kf.max() <= 65, (per_kf.min(), per_kf.max())
    P, left_out, used = gr.assemble(kfs, lms, obs, FX, FY, CX, CY)
    per_lm = np.bincount(P["lm_idx"], minlength=P["L"])
    print(f"map: {P['K']} keyframes, {P['L']} landmarks, {len(P['cam_idx'])} observations in the problem, {left_out} left out; "
          f"{per_kf.min()}..{per_kf.max()} observations per keyframe, median {np.median(per_lm[per_lm > 0])} per landmark")
    assert left_out > 0 and (~used).any() and np.median(per_lm[per_lm > 0]) >= 6

    capped = mb.global_bundle_adjust(max_iterations=1)
    assert capped["summary"].ba.termination == 1 and capped["summary"].ba.num_iterations == 1
    _same_bytes(_tables(mb), before)

    out = mb.global_bundle_adjust()
    s = out["summary"].ba
    assert (out["n_cameras"], out["n_landmarks"], out["n_observations"], out["n_left_out"]) == (P["K"], P["L"], len(P["cam_idx"]), left_out)
    assert s.linear_solver == 3 and s.termination == 0 and s.final_cost < s.initial_cost and out["summary"].pcg_iterations >= 1
    g = BAProblem(P)
    sg = g.solve_global().ba
    print(f"cost {s.initial_cost!r} -> {s.final_cost!r} in {s.num_iterations} iterations, {out['summary'].pcg_iterations} PCG iterations")
    assert (sg.initial_cost, sg.final_cost, sg.num_iterations) == (s.initial_cost, s.final_cost, s.num_iterations)
    q, t, X = g.parameters()
    lms2, obs2, kfs2 = _tables(mb)
    assert kfs2["R"][0].tobytes() == kfs["R"][0].tobytes() and kfs2["t"][0].tobytes() == kfs["t"][0].tobytes()
    for k in range(1, NKF):
        R, tt = gr.pose_to_rt(q[k], t[k])
        assert kfs2["R"][k].tobytes() == R.tobytes() and kfs2["t"][k].tobytes() == tt.tobytes(), k
        assert kfs2["R"][k].tobytes() != kfs["R"][k].tobytes()
    assert lms2["xyz"][used].tobytes() == X[used].astype(np.float32).tobytes()
    assert lms2["xyz"][~used].tobytes() == lms["xyz"][~used].tobytes()
    assert (lms2["xyz"][used] != lms["xyz"][used]).any()
    for a, b in ((lms, lms2), (obs, obs2), (kfs, kfs2)):                      # nothing else moved
        for k in a:
            if k not in ("xyz", "R", "t"):
                assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k
    mb.close()


def test_global_ba_after_a_closed_loop_with_fusion(gpu):
    """the loop-closing scene closed with fusion (observations re-pointed at the surviving landmarks), then global BA on the fused map"""
    from dvslam_amd import PoseGraph
    from dvslam_amd.backend import MappingBackend
    mb = MappingBackend(lc.FX, lc.FY, lc.CX, lc.CY, filtered=(), initial_capacity=64)
    for kf in lc.scene()[0]:
        lc.add(mb, kf)
    pg = PoseGraph()
    closed = mb.close_loop(pg, lc.scene_loop(), lc.ODO_W, fuse={})
    pg.close()
    assert closed["summary"].termination == 0 and closed["n_fused"] > 0
    lms, obs, kfs = _tables(mb)
    P, left_out, used = gr.assemble(kfs, lms, obs, lc.FX, lc.FY, lc.CX, lc.CY)
    pairs = P["cam_idx"].astype(np.int64) * P["L"] + P["lm_idx"]
    q_slot = len(kfs["frame_id"]) - 1
    shared = np.intersect1d(P["lm_idx"][P["cam_idx"] == q_slot], P["lm_idx"][P["cam_idx"] <= 2])
    print(f"fused map: {closed['n_fused']} fused, {len(pairs) - len(np.unique(pairs))} repeated (keyframe, landmark) pairs, "
          f"{len(shared)} landmarks shared by the query keyframe and the entry keyframes")
    assert len(shared) >= closed["n_fused"] > 0                               # the fusion's observations tie the loop's two ends
    out = mb.global_bundle_adjust(max_iterations=100)
    s = out["summary"].ba
    print(f"cost {s.initial_cost!r} -> {s.final_cost!r}, termination {s.termination}, {s.num_iterations} iterations")
    assert (out["n_cameras"], out["n_landmarks"], out["n_observations"], out["n_left_out"]) == (P["K"], P["L"], len(P["cam_idx"]), left_out)
    assert s.termination == 0 and s.final_cost < s.initial_cost
    assert mb.keyframes()["R"][0].tobytes() == kfs["R"][0].tobytes()
    mb.close()


def test_argument_errors_leave_the_map_unchanged(gpu):
    from dvslam_amd import DvsError
    from dvslam_amd.backend import MappingBackend
    mb = MappingBackend(FX, FY, CX, CY, filtered=(), initial_capacity=64)
    kf = arc_keyframes()[0]
    lc.add(mb, kf)
    before = _tables(mb)
    with pytest.raises(DvsError) as e:                                       # one keyframe
        mb.global_bundle_adjust()
    assert e.value.code == -6
    far = dict(kf, frame_id=900, stamp=(500, 0), xyz=kf["xyz"] + 50.0, desc=np.bitwise_xor(kf["desc"], np.uint8(255)))
    lc.add(mb, far)                                                           # two keyframes, no landmark seen twice
    before = _tables(mb)
    with pytest.raises(DvsError) as e:
        mb.global_bundle_adjust()
    assert e.value.code == -6
    with pytest.raises(TypeError):
        mb.global_bundle_adjust(etta=0.5)
    _same_bytes(_tables(mb), before)
    mb.close()
