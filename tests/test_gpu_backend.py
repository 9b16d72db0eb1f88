"""The mapping backend handle (dvs_backend_*, csrc/backend.hip) against tests/backend_ref.py, bit for bit: every table after every
keyframe, the BA window, a BA cycle, pruning in the middle of the tables, the CDR path, the tie rule and the shapes at which the
compaction kernels change trips (256 per trip), the views leave triangulation's registers (> 8 views) and the tables grow (capacity 64)."""
import struct
import numpy as np
import pytest

import backend_ref as br

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _device(gpu):
    return gpu


def _handle(**kw):
    kw.setdefault("initial_capacity", 64)   # all three tables grow mid-sequence
    return _make(kw)


def _make(kw):
    from dvslam_amd.backend import MappingBackend
    mb = MappingBackend(br.FX, br.FY, br.CX, br.CY, filtered=("person",), **kw)
    assert mb.intern("person") == br.PERSON and mb.intern("chair") == br.CHAIR and mb.intern("table") == br.TABLE
    return mb


def _ref():
    return br.BackendRef(br.FX, br.FY, br.CX, br.CY, filtered=(br.PERSON,))


def _add(x, kf):
    return x.add_keyframe(kf["frame_id"], kf["stamp"], kf["t"], kf["q"], kf["xyz"], kf["px"], kf["desc"], kf["det"])


def _same(got, want, what):
    assert set(got) == set(want), what
    for k in want:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.dtype == b.dtype and a.shape == b.shape, (what, k, a.dtype, b.dtype, a.shape, b.shape)
        if a.tobytes() != b.tobytes():
            bad = np.nonzero((a.reshape(len(a), -1) != b.reshape(len(b), -1)).any(1))[0]
            raise AssertionError(f"{what}: {k} differs in {len(bad)} rows, first {bad[0]}: {a[bad[0]]} != {b[bad[0]]}")


def _same_map(mb, ref, what):
    _same(mb.landmarks(), ref.landmark_table(), what + " landmarks")
    _same(mb.observations(), ref.observation_table(), what + " observations")
    _same(mb.keyframes(), ref.keyframe_table(), what + " keyframes")


@pytest.fixture(scope="module")
def scene():
    return br.make_scene()


@pytest.fixture(scope="module")
def ref_run(scene):
    """the restatement over the whole scene, computed once: the result record and the three tables after every keyframe"""
    ref = _ref()
    snaps = []
    for kf in scene:
        r = _add(ref, kf)
        snaps.append((r, ref.landmark_table(), ref.observation_table(), ref.keyframe_table(), ref.window_table()))
    assert ref.ties == 0, "fixture condition: the restatement must see no exact tie among candidates on this scene"
    return snaps


def test_sequence_bit_for_bit(scene, ref_run):
    mb = _handle()
    for k, kf in enumerate(scene):
        r = _add(mb, kf)
        want, lms, obs, kfs, win = ref_run[k]
        assert r == want, (k, r, want)
        _same(mb.landmarks(), lms, f"keyframe {k} landmarks")
        _same(mb.observations(), obs, f"keyframe {k} observations")
        _same(mb.keyframes(), kfs, f"keyframe {k} keyframes")
        _same(mb.window(), win, f"keyframe {k} window")
    assert ref_run[-1][1]["observation_count"].max() > 8, "the scene must reach triangulation's scratch path (> 8 views)"
    assert sum(s[0]["n_moved"] for s in ref_run) > 50 and len(ref_run[-1][1]["id"]) > 64 * 4, "tables must grow, landmarks must move"
    c = mb.counts()
    assert c["n_keyframes"] == len(scene) and c["next_observation_id"] == ref_run[-1][0]["first_observation_id"] + ref_run[-1][0]["n_kept"]
    mb.close()


def test_repeated_frame_id_is_an_argument_error(scene):
    from dvslam_amd import DvsError
    mb = _handle()
    _add(mb, scene[0])
    with pytest.raises(DvsError) as e:
        _add(mb, scene[0])
    assert e.value.code == -6
    assert mb.counts()["n_keyframes"] == 1
    mb.close()


def test_prune_in_the_middle_then_two_more_keyframes(scene):
    mb, ref = _handle(), _ref()
    for kf in scene[:8]:
        _add(mb, kf); _add(ref, kf)
    now = (scene[2]["stamp"][0] + 20, scene[2]["stamp"][1] + 1)     # landmarks last seen in keyframes 0 .. 2 are older than 20 s
    want = ref.prune(now)
    assert mb.prune(now) == want and want[0] > 20
    ids = ref.landmark_table()["id"]
    assert ids[0] < 50 and (np.diff(ids.astype(np.int64)) > 1).sum() > 5, "the prune must leave holes in the middle of the table"
    _same_map(mb, ref, "after prune")
    _same(mb.window(), ref.window_table(), "window after prune")
    for kf in scene[8:]:
        assert _add(mb, kf) == _add(ref, kf)
        _same_map(mb, ref, "keyframe after prune")
    assert ref.ties == 0
    mb.close()


def test_ba_cycle(scene):
    from dvslam_amd import SlidingWindowBA
    mb, ref = _handle(), _ref()
    for kf in scene[:6]:
        _add(mb, kf); _add(ref, kf)
    kfs, obs, lms = ref.window()
    res = SlidingWindowBA(br.FX, br.FY, br.CX, br.CY).optimize(
        [(k["frame"], k["R"].reshape(3, 3), k["t"]) for k in kfs], [(l["id"], l["cls"], l["pos"].astype(np.float64), False) for l in lms],
        [((float(o["px"][0]), float(o["px"][1])), o["lm"], o["cls"], o["frame"]) for o in obs], 20)
    if res["success"]:
        ref.apply_optimized(res["optimized_poses"], res["optimized_landmarks"])
    now = (scene[5]["stamp"][0] + 30, 0)
    want_pruned = ref.prune(now)
    got, pruned = mb.bundle_adjust(now)
    assert got["success"] == res["success"] and got["final_cost"] == res["final_cost"] and got["iterations_completed"] == res["iterations_completed"]
    assert res["success"], res["message"]
    assert pruned == want_pruned and pruned[0] > 0
    _same_map(mb, ref, "after the BA cycle")
    mb.close()


def _pack_cdr(kf):
    """Keyframe.msg as rmw serialises it (little-endian XCDR1; the layout is stated in csrc/frontend.hip)"""
    fid = b"camera_link\0"
    b = bytearray(struct.pack("<iII", kf["stamp"][0], kf["stamp"][1], len(fid)) + fid)
    b += b"\0" * (-len(b) % 8)
    b += struct.pack("<Q7d", kf["frame_id"], *kf["t"], *kf["q"])
    n = len(kf["px"])
    b += struct.pack("<I", n)
    for i in range(n):
        b += b"\0" * (-len(b) % 8)
        b += struct.pack("<Q3d", i, *kf["xyz"][i])
    b += b"\0" * (-len(b) % 4) + struct.pack("<I", n)
    for i in range(n):
        b += b"\0" * (-len(b) % 8)
        b += struct.pack("<Q2dI", i, kf["px"][i][0], kf["px"][i][1], 32) + bytes(kf["desc"][i])
    return b"\0\1\0\0" + bytes(b)


def test_cdr_path_equals_flat_arrays(scene):
    a, b = _handle(), _handle()
    for kf in scene[:4]:
        det = [(d[0], d[1], d[2], d[3], d[4]) for d in kf["det"]]
        assert b.add_keyframe_cdr(_pack_cdr(kf), det) == _add(a, kf)
        _same(b.landmarks(), a.landmarks(), "CDR landmarks"); _same(b.observations(), a.observations(), "CDR observations")
        _same(b.keyframes(), a.keyframes(), "CDR keyframes")
    a.close(); b.close()


def test_cdr_of_publish_keyframe_feeds_the_backend():
    """the front end's own payload (dvs_publish_keyframe: depth gate, back-projection, CDR) into add_keyframe_cdr == its unpacked arrays into add_keyframe"""
    from dvslam_amd import FrontendGlue, KP_DTYPE
    from dvslam_amd.glue import unpack_keyframe
    rng = np.random.default_rng(11)
    n = 300
    kps = np.zeros(n, KP_DTYPE)
    kps["x"] = rng.integers(10, 630, n); kps["y"] = rng.integers(10, 470, n); kps["size"] = 31.0
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    depth = rng.integers(200, 3500, (480, 640)).astype(np.uint16)          # some keypoints fail the 0.3 .. 3.0 m gate
    glue = FrontendGlue()
    a, b = _handle(), _handle()
    det = [(200.0, 200.0, 150.0, 150.0, "person"), (400.0, 240.0, 200.0, 300.0, "chair")]
    for k in range(2):                                                       # the second keyframe re-observes the first one's landmarks
        payload, m = glue.publish_keyframe(kps, desc, depth, br.FX, br.FY, br.CX, br.CY, np.eye(3), np.zeros(3), stamp=(k, 5), keyframe_id=40 + k)
        u = unpack_keyframe(payload)
        assert 0 < m < n and len(u["obs_pixels"]) == m
        r = b.add_keyframe_cdr(payload, det)
        assert r == a.add_keyframe(u["keyframe_id"], u["stamp"], u["translation"], u["rotation_xyzw"], u["landmark_xyz"], u["obs_pixels"], u["obs_desc"], det)
        _same(b.landmarks(), a.landmarks(), "landmarks"); _same(b.observations(), a.observations(), "observations"); _same(b.keyframes(), a.keyframes(), "keyframes")
    assert r["n_associated"] > 0 and r["n_filtered"] > 0 and b.keyframes()["frame_id"].tolist() == [40, 41]
    a.close(); b.close(); glue.close()


def test_handle_best_equals_the_entry_points_it_replaces(scene):
    """For class 0 of keyframe 5: the landmark each observation is given by the handle == the restatement's == dvs_triangulate_landmarks once
    + dvs_associate per observation in order (a matched landmark takes its triangulated position before the next observation), driven by the
    restatement's arrays as a caller of those entry points would rebuild them."""
    from dvslam_amd import FrontendGlue
    import triangulate_ref as tr
    mb, ref = _handle(), _ref()
    for kf in scene[:5]:
        _add(mb, kf); _add(ref, kf)
    kf = scene[5]
    lms = [ref.db[0][i] for i in sorted(ref.db[0])]
    by_id = {o["id"]: o for o in ref.obs}
    kf_of = {k["frame"]: j for j, k in enumerate(ref.kfs)}
    offs = [0]; vkf = []; vpx = []
    for lm in lms:
        for oid in lm["obs_ids"]:
            vkf.append(kf_of[by_id[oid]["frame"]]); vpx.append(by_id[oid]["px"])
        offs.append(len(vkf))
    R = np.array([k["R"] for k in ref.kfs]); t = np.array([k["t"] for k in ref.kfs])
    glue = FrontendGlue()
    xyz = np.array([lm["pos"] for lm in lms], np.float32)
    tri, status = glue.triangulate_landmarks(R, t, br.FX, br.FY, br.CX, br.CY, offs, np.array(vkf, np.int32), np.array(vpx, np.float32), xyz)
    desc = np.array([lm["desc"] for lm in lms], np.uint8)
    Rk = br.quat_to_R(kf["q"])
    want = []
    for i in range(len(kf["px"])):
        px = kf["px"][i].astype(np.float32)
        if br.categorize(px, kf["det"]) != 0:
            continue
        j = int(glue.associate(kf["desc"][i:i + 1], px[None], desc, xyz, Rk, kf["t"], br.FX, br.FY, br.CX, br.CY)[0])
        want.append(lms[j]["id"] if j >= 0 else -1)
        if j >= 0 and status[j] == tr.UPDATED:
            xyz[j] = tri[j]
    r = _add(mb, kf); _add(ref, kf)
    ob = mb.observations()
    mine = (ob["frame_id"] == kf["frame_id"]) & (ob["class_id"] == 0)
    got = [int(l) if l < r["first_landmark_id"] else -1 for l in ob["landmark_id"][mine]]
    assert got == ref.last_best[0] == want
    assert sum(b >= 0 for b in want) > 30 and (status == tr.UPDATED).sum() > 10 and ref.ties == 0
    mb.close(); glue.close()


def _two_views(n, seed):
    """n points seen from two poses, unlabeled: the second keyframe matches all of them against n landmarks"""
    rng = np.random.default_rng(seed)
    X = np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(-1.0, 1.0, n), rng.uniform(2.5, 4.5, n)], 1)
    D = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    out = []
    for k in range(2):
        t = np.array([0.3 * k, 0.0, 0.0])
        u = br.FX * (-X[:, 0] + t[0]) / X[:, 2] + br.CX; v = br.FY * (-X[:, 1] + t[1]) / X[:, 2] + br.CY
        px = np.stack([u, v], 1) + rng.normal(0, 0.2, (n, 2))
        out.append(dict(frame_id=k, stamp=(k, 0), t=t, q=br.Q_Z180, xyz=X + rng.normal(0, 0.02, (n, 3)), px=px, desc=D.copy(),
                        det=[(320.0, 240.0, 100.0, 480.0, br.CHAIR)] if n else []))
    return out


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1025])
def test_observation_counts_around_the_trip_size(n):
    mb, ref = _handle(), _ref()
    for kf in _two_views(n, 100 + n):
        assert _add(mb, kf) == _add(ref, kf)
        _same_map(mb, ref, f"n = {n}")
    assert ref.ties == 0
    if n >= 63:
        assert ref.landmark_table()["observation_count"].max() == 2
    mb.close()


def test_all_filtered_new_class_and_double_match():
    mb, ref = _handle(), _ref()
    kfs = _two_views(40, 5)
    whole = [(320.0, 240.0, 1e6, 1e6, br.PERSON)]                    # the points are not confined to the image
    k0 = dict(kfs[0]); k0["det"] = []
    k1 = dict(kfs[1]); k1["det"] = whole; k1["frame_id"] = 7                  # every observation filtered: an empty keyframe joins the map
    k2 = dict(kfs[1]); k2["det"] = [(320.0, 240.0, 1e6, 1e6, br.TABLE)]; k2["frame_id"] = 8   # a class with no landmarks yet
    k3 = dict(kfs[1]); k3["det"] = []; k3["frame_id"] = 9
    k3["px"] = np.concatenate([kfs[1]["px"], kfs[1]["px"][:5]]); k3["xyz"] = np.concatenate([kfs[1]["xyz"], kfs[1]["xyz"][:5]])
    k3["desc"] = np.concatenate([kfs[1]["desc"], kfs[1]["desc"][:5]])       # five landmarks matched twice within one keyframe
    for kf in (k0, k1, k2, k3):
        r = _add(mb, kf)
        assert r == _add(ref, kf)
        _same_map(mb, ref, f"frame {kf['frame_id']}")
    assert ref.kfs[1]["obs_ids"] == [] and ref.ties == 0 and br.TABLE in ref.db
    assert ref.landmark_table()["observation_count"].max() == 3, "no landmark was matched twice within the last keyframe"
    mb.close()


def test_tie_rule_lowest_id_wins():
    mb = _handle()
    d = np.full((1, 32), 0x5A, np.uint8)
    X = np.array([[0.2, 0.1, 3.0]])
    px = np.array([[br.FX * -0.2 / 3.0 + br.CX, br.FY * -0.1 / 3.0 + br.CY]])
    mb.add_keyframe(0, (0, 0), (0, 0, 0), br.Q_Z180, np.repeat(X, 2, 0), np.repeat(px, 2, 0), np.repeat(d, 2, 0))
    r = mb.add_keyframe(1, (1, 0), (0, 0, 0), br.Q_Z180, X, px, d)
    assert r["n_associated"] == 1 and r["n_created"] == 0
    lm = mb.landmarks(); ob = mb.observations()
    assert lm["id"].tolist() == [0, 1] and lm["xyz"][0].tobytes() == lm["xyz"][1].tobytes()
    assert ob["landmark_id"].tolist() == [0, 1, 0] and lm["observation_count"].tolist() == [2, 1]
    mb.close()
