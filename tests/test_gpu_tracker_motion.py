"""The tracker's motion-mask opt-in (dvs_tracker_set_motion_mask, csrc/tracker.hip) on scene 2 of tests/motion_ref.py: the canvas plane at
1500 mm along synth.traj_pose, 640 x 480, 12 frames, lag 4, and a 120 x 160 px block at 900 mm that moves 36 px per frame with a texture
of its own.  The mask the tracker used is recomputed by the numpy reference from the two depth frames and the returned relative pose, the
pose from the returned R_, t_ history; with the feature off, or on over a static scene, the run is the plain tracker's bit for bit."""
import numpy as np
import pytest
import motion_ref as mr

COLS, ROWS, F, NF, LAG, N = 640, 480, 600.0, 1000, 4, 12
CX, CY = COLS / 2.0, ROWS / 2.0
pytestmark = pytest.mark.gpu


def _tracker(motion):
    from dvslam_amd import tracker as T, motion as M
    tr = T.Tracker(T.default_params(ROWS, COLS, F, F, CX, CY, nfeatures=NF))
    if motion:
        tr.set_motion_mask(M.default_params(), LAG)
    return tr


def _run(tr, frames, depths):
    """tracker_ref.run_tracker plus, per frame, what the extraction used and the backend features"""
    out = []
    for t, (img, depth) in enumerate(zip(frames, depths)):
        r, payload = tr.track(img, depth, (t, 0))
        k, _, sel = tr.backend_features()
        r["payload"] = payload; r["sel"] = sel.astype(np.int64); r["bk"] = k
        r["mask"], r["mR"], r["mt"], r["ref"], r["mstats"] = tr.motion_mask()
        out.append(r)
    return out


def _in_box(k, box, margin=0):
    x0, y0, w, h = box
    return (k["x"] >= x0 - margin) & (k["x"] < x0 + w + margin) & (k["y"] >= y0 - margin) & (k["y"] < y0 + h + margin)


@pytest.fixture(scope="module")
def block_scene():
    return mr.scene2(N, COLS, ROWS, block=True)


@pytest.fixture(scope="module")
def block_runs(gpu, block_scene):
    frames, depths, _ = block_scene
    on, off = _tracker(True), _tracker(False)
    runs = dict(on=_run(on, frames, depths), off=_run(off, frames, depths))
    on.reset()
    runs["again"] = _run(on, frames, depths)
    on.set_motion_mask(None)
    on.reset()
    runs["switched_off"] = _run(on, frames, depths)
    on.close(); off.close()
    return runs


def test_static_scene_masks_nothing_and_equals_the_plain_tracker(gpu):
    import tracker_ref as ref
    frames, depths, _ = mr.scene2(N, COLS, ROWS, block=False)
    on, off = _tracker(True), _tracker(False)
    got, want = _run(on, frames, depths), _run(off, frames, depths)
    on.close(); off.close()
    assert ref.first_difference(got, want) is None, ref.first_difference(got, want)
    assert [r["ref"] for r in got] == [-1] + [t - min(LAG, t) for t in range(1, N)] and all(r["ref"] == -1 for r in want)
    for t, r in enumerate(got[1:], 1):
        assert r["mstats"]["n_masked"] == 0 and r["mstats"]["n_seed"] == 0 and r["mstats"]["n_valid"] > ROWS * COLS // 2, (t, r["mstats"])
        assert (r["mask"] == 255).all() and r["pose_updated"] == 1
    assert all(r["bk"].tobytes() == w["bk"].tobytes() for r, w in zip(got, want))


def test_mask_is_the_references_on_the_returned_pose(block_scene, block_runs):
    frames, depths, boxes = block_scene
    got = block_runs["on"]
    assert [r["ref"] for r in got] == [-1] + [t - min(LAG, t) for t in range(1, N)]
    assert (got[0]["mask"] == 255).all() and got[0]["mstats"]["n_valid"] == 0
    for t in range(5, N):
        r = got[t]
        want = mr.segment(depths[r["ref"]], depths[t], (F, F, CX, CY), r["mR"], r["mt"])
        assert (r["mask"] == want["mask"]).all() and r["mstats"] == want["stats"], (t, r["mstats"], want["stats"])
        # the pose it was made with: constant velocity from the returned history, against the reference frame's pose
        R1, t1, R2, t2 = got[t - 1]["R"], got[t - 1]["t"], got[t - 2]["R"], got[t - 2]["t"]
        if got[t - 1]["pose_updated"]:
            Rp, tp = R1 @ (R2.T @ R1), R1 @ (R2.T @ (t1 - t2)) + t1
        else:
            Rp, tp = R1, t1
        Rr, tr_ = got[r["ref"]]["R"], got[r["ref"]]["t"]
        assert np.abs(r["mR"] - Rr.T @ Rp).max() <= 1e-12 and np.abs(r["mt"] - Rr.T @ (tp - tr_)).max() <= 1e-12, t
        # every block pixel is masked, nothing more than 8 px outside it is
        x0, y0, w, h = boxes[t]
        assert (r["mask"][y0:y0 + h, x0:x0 + w] == 0).all(), t
        outside = r["mask"].copy(); outside[max(y0 - 8, 0):y0 + h + 8, max(x0 - 8, 0):x0 + w + 8] = 255
        assert (outside == 255).all(), t
    assert sum(r["pose_updated"] for r in got) >= N - 2


def test_no_feature_on_the_block(block_scene, block_runs):
    from dvslam_amd import ORBextractor
    frames, depths, boxes = block_scene
    on, off = block_runs["on"], block_runs["off"]
    orb = ORBextractor(NF, 1.2, 8, 20, 7)
    for t in range(5, N):
        n, k, _ = orb.extract_masked(frames[t], on[t]["mask"])       # the extraction the tracker made: the same entry point, image and mask
        n0, k0, _ = orb(frames[t])
        assert n == on[t]["n_extracted"] and n0 == off[t]["n_extracted"], t
        print(t, "in the block: extracted", int(_in_box(k, boxes[t]).sum()), "/", int(_in_box(k0, boxes[t]).sum()), "backend",
              int(_in_box(on[t]["bk"], boxes[t]).sum()), "/", int(_in_box(off[t]["bk"], boxes[t]).sum()))
        assert not _in_box(k, boxes[t]).any() and not _in_box(on[t]["bk"], boxes[t]).any(), t
        assert _in_box(k0, boxes[t]).sum() >= 20 and _in_box(off[t]["bk"], boxes[t]).sum() >= 20, t   # ... which the plain run does put there
        assert on[t]["n_backend"] > 100


def test_reset_repeats_and_switching_off_restores_the_plain_run(block_runs):
    import tracker_ref as ref
    on, again, off, sw = (block_runs[k] for k in ("on", "again", "off", "switched_off"))
    assert ref.first_difference(again, on) is None, ref.first_difference(again, on)
    for a, b in zip(again, on):
        assert a["mask"].tobytes() == b["mask"].tobytes() and a["mR"].tobytes() == b["mR"].tobytes() and a["mt"].tobytes() == b["mt"].tobytes()
        assert a["ref"] == b["ref"] and a["mstats"] == b["mstats"] and a["bk"].tobytes() == b["bk"].tobytes()
    assert ref.first_difference(sw, off) is None, ref.first_difference(sw, off)
    assert all(r["ref"] == -1 and (r["mask"] == 255).all() and r["bk"].tobytes() == w["bk"].tobytes() for r, w in zip(sw, off))
    assert ref.first_difference(on, off) is not None                  # the mask changed the run it was switched on for


def test_tracking_reset_begins_a_new_sequence(gpu):
    """a blank image at frame 3: no features -> tracking reset, and again at 4 (prev_kps_ empty).  A reset frame begins a sequence, the frame
    after a reset is extracted unmasked, and the references never reach behind the last reset"""
    import tracker_ref as ref
    frames, depths, _ = mr.scene2(8, COLS, ROWS, block=False)
    frames[3] = np.zeros((ROWS, COLS), np.uint8)
    on, off = _tracker(True), _tracker(False)
    got, want = _run(on, frames, depths), _run(off, frames, depths)
    on.close(); off.close()
    assert [r["tracking_reset"] for r in got] == [0, 0, 0, 1, 1, 0, 0, 0]
    assert [r["ref"] for r in got] == [-1, 0, 0, 0, -1, -1, 4, 4]
    assert ref.first_difference(got, want) is None, ref.first_difference(got, want)
    assert all(r["mstats"]["n_masked"] == 0 for r in got)


def test_lag_outside_its_range_is_refused(gpu):
    from dvslam_amd import motion as M, DvsError
    tr = _tracker(False)
    for lag in (0, 17):
        with pytest.raises(DvsError) as e:
            tr.set_motion_mask(M.default_params(), lag)
        assert e.value.code == -6
    with pytest.raises(DvsError):
        tr.set_motion_mask(M.default_params(dilate_radius=32), 4)
    tr.close()
