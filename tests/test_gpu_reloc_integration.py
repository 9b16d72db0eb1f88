"""Relocalisation through the handles that own the data: dvs_tracker_relocalize over the tracker's last depth-filtered features and the
backend's landmark table after a reset — as a dry run, which must leave the tracker as it was, and applied, after which the next frame's
odometry composes on the found pose —, dvs_backend_relocalize_frame against dvs_reloc_locate_device on the arrays the getters return, and
a tracker that never relocalises beside a relocaliser that exists."""
import numpy as np
import pytest
import reloc_ref as rr

pytestmark = pytest.mark.gpu
COLS, ROWS, F = 640, 480, 600.0


def _same(a, b):
    return set(a) == set(b) and all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a)


@pytest.fixture(scope="module")
def world(gpu):
    """a tracker, a backend holding the keyframes of frames 0 .. 2, a map tracker and a relocaliser; the tracker's results on the four frames"""
    from dvslam_amd import synth, tracker as T, map_track as M, reloc as RL
    from dvslam_amd.backend import MappingBackend
    frames = [synth.make_traj_frame(t, COLS, ROWS, seed=1234) for t in range(4)]
    depth = np.full((ROWS, COLS), 1500, np.uint16)
    tr = T.Tracker(T.default_params(ROWS, COLS, F, F, COLS / 2.0, ROWS / 2.0, nfeatures=500))
    mb = MappingBackend(F, F, COLS / 2.0, ROWS / 2.0, filtered=())
    mt = M.MapTracker(M.default_params(ROWS, COLS, F, F, COLS / 2.0, ROWS / 2.0))
    plain, payloads = [], []
    for i, f in enumerate(frames):
        r, payload = tr.track(f, depth, (i, 0))
        plain.append(r); payloads.append(payload)
        if payload is not None and i < 3:
            mb.add_keyframe_cdr(payload)
    assert mb.counts()["n_keyframes"] >= 2 and mb.counts()["n_landmarks"] > 100
    rl = RL.Relocalizer(RL.default_params(F, F, COLS / 2.0, ROWS / 2.0))
    w = dict(frames=frames, depth=depth, tr=tr, mb=mb, mt=mt, rl=rl, plain=plain, payloads=payloads)
    yield w
    rl.close(); tr.close(); mt.close(); mb.close()


def _lost_then_frame2(w):
    """the tracker reset, then frame 2: its state is the identity pose and frame 2's features"""
    w["tr"].reset()
    r, _ = w["tr"].track(w["frames"][2], w["depth"], (2, 0))
    assert r["first_frame"] == 1 and np.array_equal(r["R"], np.eye(3)) and not r["t"].any()
    return r


def test_relocalize_dry_run_and_applied(world):
    w = world
    tr, mb, mt, rl, plain = w["tr"], w["mb"], w["mt"], w["rl"], w["plain"]
    before = (mb.landmarks(), mb.observations(), mb.keyframes())
    # without any relocalisation: frame 3 after the reset
    _lost_then_frame2(w)
    a3, _ = tr.track(w["frames"][3], w["depth"], (3, 0))
    # the dry run changes nothing
    _lost_then_frame2(w)
    dry = tr.relocalize(mb, rl, mt, apply=False)
    assert dry["status"] == rr.OK and dry["track"]["n_inliers"] >= 30 and dry["n_pairs"] >= 20
    b3, _ = tr.track(w["frames"][3], w["depth"], (3, 0))
    assert _same(a3, b3)
    # the found pose is frame 2's pose in the map (the map itself carries a centimetre of noise)
    assert np.abs(dry["R"] - plain[2]["R"]).max() < 0.01 and np.abs(dry["t"] - plain[2]["t"]).max() < 0.03
    # applied: the tracker's pose is the found one, and frame 3 composes its motion on it
    _lost_then_frame2(w)
    res = tr.relocalize(mb, rl, mt, apply=True)
    assert res["raw"] == dry["raw"]                                                  # the same call twice: the same bytes
    c3, _ = tr.track(w["frames"][3], w["depth"], (3, 0))
    assert c3["pose_updated"] == 1 and a3["pose_updated"] == 1
    assert c3["rvec"].tobytes() == a3["rvec"].tobytes() and c3["tvec"].tobytes() == a3["tvec"].tobytes()     # the odometry itself is the same
    Ri, ti = a3["R"], a3["t"]                                                        # frame 3's motion: a3 composed it on the identity
    assert np.abs(c3["R"] - res["R"] @ Ri).max() < 1e-12 and np.abs(c3["t"] - (res["t"] + res["R"] @ ti)).max() < 1e-12
    assert c3["R"].tobytes() != a3["R"].tobytes()
    after = (mb.landmarks(), mb.observations(), mb.keyframes())
    for x, y in zip(before, after):                                                  # the map is not modified
        assert set(x) == set(y) and all(np.asarray(x[k]).tobytes() == np.asarray(y[k]).tobytes() for k in x)


def test_before_the_first_frame_and_after_a_frame_without_features(world):
    from dvslam_amd._lib import DvsError
    w = world
    tr, mb, mt, rl = w["tr"], w["mb"], w["mt"], w["rl"]
    tr.reset()
    with pytest.raises(DvsError) as e:
        tr.relocalize(mb, rl, mt)
    assert e.value.code == -1                                                        # DVS_ERR_EMPTY
    _lost_then_frame2(w)
    r, _ = tr.track(w["frames"][3], np.zeros((ROWS, COLS), np.uint16), (3, 0))       # no depth anywhere: nothing survives the depth filter
    assert r["tracking_reset"] == 1 and r["n_filtered"] == 0
    res = tr.relocalize(mb, rl, mt, apply=True)
    assert res["status"] == rr.FEW_PAIRS and res["n_pairs"] == 0 and np.array_equal(res["R"], np.eye(3))


def test_backend_relocalize_frame_equals_locate_device_on_the_getters_arrays(world):
    from dvslam_amd._lib import DeviceBuffer
    w = world
    tr, mb, mt, rl = w["tr"], w["mb"], w["mt"], w["rl"]
    _lost_then_frame2(w)
    kps, kd = tr.filtered_features()
    lm = mb.landmarks()
    ids = np.ascontiguousarray(lm["id"]).astype(np.int64)
    arrays = [np.ascontiguousarray(lm["xyz"], np.float32), np.ascontiguousarray(lm["desc"], np.uint8), ids, kps, kd]
    bufs = [DeviceBuffer(a.nbytes).upload(a) for a in arrays]
    direct = rl.locate_device(mt, bufs[0], bufs[1], bufs[2], len(ids), bufs[3], bufs[4], len(kps))
    pairs = rl.pairs()
    through = mb.relocalize_frame(rl, mt, bufs[3], bufs[4], len(kps))
    assert through["raw"] == direct["raw"] and direct["status"] == rr.OK
    assert all(a.tobytes() == b.tobytes() for a, b in zip(pairs, rl.pairs()))
    assert through["raw"] == tr.relocalize(mb, rl, mt)["raw"]                        # and the tracker's form hands over the same arrays
    for b in bufs:
        b.free()


def test_a_tracker_that_never_relocalises_is_unchanged_beside_one(world):
    from dvslam_amd import tracker as T
    w = world
    other = T.Tracker(T.default_params(ROWS, COLS, F, F, COLS / 2.0, ROWS / 2.0, nfeatures=500))      # created with a dvs_reloc alive beside it
    for i, f in enumerate(w["frames"]):
        r, payload = other.track(f, w["depth"], (i, 0))
        assert _same(r, w["plain"][i]) and payload == w["payloads"][i], i
    other.close()
