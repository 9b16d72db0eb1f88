"""Loop closing on the map (dvs_backend_get_anchors / _build_pose_graph / _close_loop / _fuse, csrc/loop_close.hip) against
tests/loop_closing_ref.py, bit for bit unless a test says otherwise: anchors after every keyframe and after a prune, the graph the keyframes
imply, close_loop against the composition of its parts, fusion dry and applied on the scene (then two more keyframes), the shapes at which
the propose and compaction kernels change trips (256 per LDS tile and per workgroup), the special cases of the rule on a hand-built map,
determinism and argument errors.

Three cases cannot be reached through the public entry points and are held on the restatement in tests/test_loop_closing_cpu.py instead:
a landmark without any observation (anchor -1) and an observation whose landmark left the table (dvs_backend_prune removes a landmark
together with every observation naming it), and a removed landmark in the FIRST table row (the removed id is the higher of its pair, so
the lowest it can be is the second row: _pair_map(1, 1) removes exactly that one).  No failing solve is tested: pose_graph_ref names no
inexpensive failing case, and a loop edge with a rotation error of pi converges on the restatement instead of failing."""
import ctypes as C
import numpy as np
import pytest

import backend_ref as br
import loop_closing_ref as lc

pytestmark = pytest.mark.gpu
Z180 = br.Q_Z180


@pytest.fixture(autouse=True)
def _device(gpu):
    return gpu


def _handle(**kw):
    from dvslam_amd.backend import MappingBackend
    kw.setdefault("initial_capacity", 64)
    return MappingBackend(lc.FX, lc.FY, lc.CX, lc.CY, filtered=(), **kw)


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


def _tables(mb):
    return mb.landmarks(), mb.observations(), mb.keyframes()


def _same_tables(a, b, what):
    for x, y, name in zip(a, b, ("landmarks", "observations", "keyframes")):
        _same(x, y, f"{what} {name}")


def _same_fuse(got, want, what):
    for k in ("n_sources", "n_targets", "n_proposals", "n_fused"):
        assert got[k] == want[k], (what, k, got[k], want[k])
    sv, rm, err = got["pairs"]
    assert sv.tolist() == [p[0] for p in want["pairs"]] and rm.tolist() == [p[1] for p in want["pairs"]], what
    assert err.tobytes() == np.array([p[2] for p in want["pairs"]], np.float64).tobytes(), what


def _scene_handle():
    mb = _handle()
    for kf in lc.scene()[0]:
        lc.add(mb, kf)
    return mb


def _entry_frames():
    return [kf["frame_id"] for kf in lc.scene()[0][:3]]


def _closed_pair():
    """the scene on a handle, closed without fusion, and the restatement given the handle's geometry"""
    from dvslam_amd import PoseGraph
    mb = _scene_handle()
    pg = PoseGraph()
    out = mb.close_loop(pg, lc.scene_loop(), lc.ODO_W)
    pg.close()
    assert out["summary"].termination == 0
    ref, _ = lc.scene_ref()
    lc.adopt_geometry(ref, mb.keyframes(), mb.landmarks())
    _same_map(mb, ref, "after close")
    return mb, ref


def test_anchors_after_every_keyframe_and_after_a_prune():
    mb = _handle()
    want = lc.scene_anchors()
    scene = lc.scene()[0]
    for k, kf in enumerate(scene):
        lc.add(mb, kf)
        ids, anc = mb.anchors()
        assert ids.dtype == np.uint64 and anc.dtype == np.int32
        assert ids.tobytes() == want[k][0].tobytes() and anc.tobytes() == want[k][1].tobytes(), k
    assert len(np.unique(want[-1][1])) == len(scene), "every keyframe must anchor some landmark"
    ref, _ = lc.scene_ref()
    now = (scene[4]["stamp"][0] + 20, 1)              # single-view landmarks last seen in keyframes 0 .. 4 are older than 20 s
    gone = ref.prune(now)
    assert mb.prune(now) == gone and gone[0] > 100
    ids, anc = lc.anchors(ref)
    assert (np.diff(ids.astype(np.int64)) > 1).sum() > 20, "the prune must leave holes in the table"
    got = mb.anchors()
    assert got[0].tobytes() == ids.tobytes() and got[1].tobytes() == anc.tobytes()
    mb.close()


def test_build_pose_graph_equals_the_restatement():
    mb = _scene_handle()
    ref, _ = lc.scene_ref()
    loops = lc.scene_loop() + [(210, 201, (0.01, -0.02, 0.03), (0.5, -2.5, 0.01), 30.0, 20.0)]
    got, want = mb.build_pose_graph(loops, lc.ODO_W), lc.build_pose_graph(ref, loops, lc.ODO_W)
    rg, rw = got.pop("rvec"), want.pop("rvec")
    _same(got, want, "pose graph")
    # a dozen FP64 operations on O(1) rotations plus one atan2, each good to an ulp or so: 1e-12 leaves two orders of magnitude
    assert rg.shape == rw.shape and np.abs(rg - rw).max() <= 1e-12
    assert rg[len(ref.kfs) - 1:].tobytes() == rw[len(ref.kfs) - 1:].tobytes(), "loop edges are passed through unchanged"
    assert len(got["ei"]) == len(ref.kfs) - 1 + 2
    mb.close()


def test_close_loop_equals_the_composition_of_its_parts():
    from dvslam_amd import PoseGraph
    mb = _scene_handle()
    loops = lc.scene_loop()
    g = mb.build_pose_graph(loops, lc.ODO_W)
    ids, anc = mb.anchors()
    before = _tables(mb)
    parts = PoseGraph()
    parts.set_nodes(g["R"], g["t"], g["fixed"]).set_edges(g["ei"], g["ej"], g["rvec"], g["tvec"], g["w_rot"], g["w_trans"])
    s2 = parts.solve()
    R2, t2 = parts.nodes()
    xyz2 = parts.correct_points(before[0]["xyz"], anc)
    pg = PoseGraph()
    out = mb.close_loop(pg, loops, lc.ODO_W)
    s = out["summary"]
    for k, _ in type(s)._fields_:
        assert getattr(s, k) == getattr(s2, k), k
    assert s.termination == 0 and s.final_cost < s.initial_cost
    assert (out["n_nodes"], out["n_edges"], out["n_landmarks_moved"]) == (len(g["fixed"]), len(g["ei"]), int((anc >= 0).sum()))
    assert (out["n_sources"], out["n_targets"], out["n_proposals"], out["n_fused"]) == (0, 0, 0, 0)
    after = _tables(mb)
    assert after[2]["R"].tobytes() == R2.tobytes() and after[2]["t"].tobytes() == t2.tobytes()
    assert after[0]["xyz"].tobytes() == xyz2.tobytes()
    assert (after[0]["xyz"] != before[0]["xyz"]).any(1).sum() > 1000, "the correction must move the map"
    # nothing but the poses and the positions changed
    want = [dict(before[0], xyz=xyz2), before[1], dict(before[2], R=R2, t=t2)]
    _same_tables(after, want, "after close")
    # the host copy of the poses follows: the graph built now starts from the new poses
    assert mb.build_pose_graph(loops, lc.ODO_W)["R"].tobytes() == R2.tobytes()
    parts.close(); pg.close(); mb.close()


def test_fusion_dry_run_on_the_scene():
    mb, ref = _closed_pair()
    q = lc.scene()[0][-1]["frame_id"]
    before = _tables(mb)
    want = lc.fuse(ref, q, _entry_frames(), apply=False)
    got = mb.fuse(q, _entry_frames(), apply=False)
    assert want["n_fused"] >= 100 and want["n_proposals"] > want["n_fused"]
    _same_fuse(got, want, "dry run")
    _same_tables(_tables(mb), before, "dry run")
    mb.close()


def test_fusion_applied_then_two_more_keyframes():
    mb, ref = _closed_pair()
    scene = lc.scene()[0]
    q = scene[-1]["frame_id"]
    nlm = mb.counts()["n_landmarks"]
    want = lc.fuse(ref, q, _entry_frames(), apply=True)
    got = mb.fuse(q, _entry_frames(), apply=True)
    _same_fuse(got, want, "applied")
    _same_map(mb, ref, "after fusion")
    c = mb.counts()
    assert c["n_landmarks"] == nlm - want["n_fused"] and c["next_landmark_id"] == ref.next_lm and c["next_observation_id"] == ref.next_obs
    removed_rows = np.searchsorted(lc.scene_ref()[0].landmark_table()["id"], got["pairs"][1])
    assert removed_rows.max() >= nlm - 10 and removed_rows.min() < nlm - 250, "removed rows over the last keyframe's part of the table"
    for k in (0, 1):                                  # the camera stays at the start: the survivors are associated again and triangulated
        kf = dict(scene[k], frame_id=300 + k, stamp=(40 + 2 * k, 0))
        assert lc.add(mb, kf) == lc.add(ref, kf)
        _same_map(mb, ref, f"keyframe {k} after fusion")
    mb.close()


def test_close_loop_with_fusion_equals_close_then_fuse_and_is_deterministic():
    from dvslam_amd import PoseGraph
    mb, ref = _closed_pair()
    scene = lc.scene()[0]
    want = lc.fuse(ref, scene[-1]["frame_id"], _entry_frames(), apply=True)
    runs = []
    for _ in range(2):
        h = _scene_handle()
        pg = PoseGraph()
        out = h.close_loop(pg, lc.scene_loop(), lc.ODO_W, fuse={})      # fuse_neighbours 2 around entry keyframe 0: keyframes 0, 1, 2
        assert [out[k] for k in ("n_sources", "n_targets", "n_proposals", "n_fused")] == [want[k] for k in ("n_sources", "n_targets", "n_proposals", "n_fused")]
        runs.append(_tables(h))
        pg.close(); h.close()
    _same_tables(runs[0], runs[1], "two identical runs")
    _same_tables(runs[0], (ref.landmark_table(), ref.observation_table(), ref.keyframe_table()), "close with fusion")
    mb.close()


# ---- hand-built maps ------------------------------------------------------------------------------------------------------------------
def _world(u, v, z=3.0):
    """the point at depth z that the camera of Z180 at the origin sees at pixel (u, v)"""
    return (-(u - lc.CX) * z / lc.FX, -(v - lc.CY) * z / lc.FY, z)


def _flip(rng, d, n):
    d = d.copy()
    for b in rng.choice(256, n, replace=False):
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


def _kf(frame, sec, xyz, px, desc, det=()):
    return dict(frame_id=frame, stamp=(sec, 0), t=np.zeros(3), q=Z180, xyz=np.array(xyz, np.float64).reshape(-1, 3), px=np.array(px, np.float64).reshape(-1, 2),
                desc=np.array(desc, np.uint8).reshape(-1, 32), det=list(det))


def _pair_map(n_q, n_src, seed, tail=True):
    """Query keyframe 2 first: n_q observations on a 30-pixel grid whose landmarks (the targets) are reported behind the camera, so nothing
    ever associates with them.  Then entry keyframe 1: n_src sources, source i placed to reproject within 2 pixels of query observation
    i % n_q with its descriptor (up to 5 bits flipped), seen at pixels far from everything.  Then (tail) keyframe 3 with three
    unrelated landmarks, so that the removed rows are in the middle of the table and not at its end."""
    rng = np.random.default_rng(seed)
    qpx = np.array([(20.0 + 30 * (k % 20), 20.0 + 30 * (k // 20)) for k in range(n_q)])
    qd = rng.integers(0, 256, (n_q, 32), dtype=np.uint8)
    kq = _kf(2, 10, [(0.1 * k, 0.0, -5.0) for k in range(n_q)], qpx, qd)
    sxyz, sd = [], []
    for i in range(n_src):
        j = i % n_q
        du, dv = rng.uniform(-2, 2, 2)
        sxyz.append(_world(qpx[j, 0] + du, qpx[j, 1] + dv)); sd.append(_flip(rng, qd[j], int(rng.integers(0, 6))))
    ke = _kf(1, 12, sxyz, [(610.0 + (i % 3), 400.0 + 0.25 * i) for i in range(n_src)], sd)
    kc = _kf(3, 14, [(5.0, 5.0, -4.0)] * 3, [(630.0, 30.0 + 10 * k) for k in range(3)], rng.integers(0, 256, (3, 32), dtype=np.uint8))
    return [kq, ke, kc] if tail else [kq, ke]


@pytest.mark.parametrize("n_q,n_src", [(1, 1), (255, 256), (256, 257), (257, 1)])
def test_tile_and_workgroup_edges(n_q, n_src):
    mb, ref = _handle(), lc.new_ref()
    tail = n_src > 1 or n_q == 1                     # (257, 1) has no tail: its one source is the last row of the table
    for kf in _pair_map(n_q, n_src, seed=n_q + n_src, tail=tail):
        r = lc.add(ref, kf)
        assert lc.add(mb, kf) == r and r["n_associated"] == 0, "hand-built map: nothing may associate"
    before = _tables(mb)
    want = lc.fuse(ref, 2, [1], apply=False)
    assert (want["n_sources"], want["n_targets"]) == (n_src, n_q) and want["n_fused"] == min(n_q, n_src) and want["n_proposals"] == n_src
    _same_fuse(mb.fuse(2, [1], apply=False), want, "dry run")
    _same_tables(_tables(mb), before, "dry run")
    assert lc.fuse(ref, 2, [1], apply=True) == want
    _same_fuse(mb.fuse(2, [1], apply=True), want, "applied")
    _same_map(mb, ref, "after fusion")
    removed_rows = np.searchsorted(before[0]["id"], [p[1] for p in want["pairs"]])
    nlm = len(before[0]["id"])
    assert removed_rows.min() >= n_q and removed_rows.max() < (nlm - 3 if tail else nlm)
    if (n_q, n_src) == (1, 1):
        assert removed_rows.tolist() == [1] and nlm == 5, "the second row of the table: the lowest a removed landmark can be"
    if not tail:
        assert removed_rows.tolist() == [nlm - 1], "the last row of the table"
    mb.close()


def test_zero_sources_zero_targets_and_an_empty_keyframe():
    rng = np.random.default_rng(5)
    px = np.array([(100.0 + 40 * k, 200.0) for k in range(5)])
    d = rng.integers(0, 256, (5, 32), dtype=np.uint8)
    xyz = [_world(u, v) for u, v in px]
    kfs = [_kf(1, 10, xyz, px, d), _kf(2, 12, xyz, px + 0.5, d), _kf(3, 14, np.zeros((0, 3)), np.zeros((0, 2)), np.zeros((0, 32), np.uint8))]
    mb, ref = _handle(), lc.new_ref()
    for kf in kfs:
        assert lc.add(mb, kf) == lc.add(ref, kf)
    assert ref.next_lm == 5, "keyframe 2 must associate with every landmark of keyframe 1"
    before = _tables(mb)
    for q, E, counts in ((2, [1], (0, 5)), (3, [1, 2], (5, 0)), (1, [3], (0, 5))):
        want = lc.fuse(ref, q, E, apply=True)
        assert (want["n_sources"], want["n_targets"], want["n_proposals"], want["n_fused"]) == counts + (0, 0)
        _same_fuse(mb.fuse(q, E, apply=True), want, f"q = {q}")
        _same_tables(_tables(mb), before, f"q = {q}")
    empty = _handle()
    lc.add(empty, kfs[2]); lc.add(empty, dict(kfs[2], frame_id=4))
    got = empty.fuse(3, [4])
    assert [got[k] for k in ("n_sources", "n_targets", "n_proposals", "n_fused")] == [0, 0, 0, 0] and len(got["pairs"][0]) == 0
    empty.close(); mb.close()


def test_special_cases_of_the_rule():
    """keyframe 1 creates landmark 0 (T_a); the query keyframe 2 sees it twice (two observations naming one target) and creates the targets
    T_b (id 1), T_c (id 2), T_d (id 3) reported behind the camera; the entry keyframe 3 creates the sources S_a (4) on T_a's observations,
    S_b1 (5) and S_b2 (6) at one position (an exact tie in e: the lower id wins), S_c (7) equal to T_c's observation in everything but its
    class, and S_d (8) behind the camera with the descriptor of T_d's observation at the image corner."""
    rng = np.random.default_rng(9)
    d = rng.integers(0, 256, (4, 32), dtype=np.uint8)
    pa, pb, pc, pd = (200.0, 150.0), (400.0, 300.0), (500.0, 100.0), (1.0, 1.5)
    junk = (0.0, 0.0, -5.0)
    k1 = _kf(1, 10, [_world(*pa)], [pa], [d[0]])
    k2 = _kf(2, 12, [_world(*pa), _world(*pa), junk, junk, junk], [(pa[0] + 1, pa[1]), (pa[0], pa[1] + 2), pb, pc, pd], [d[0], d[0], d[1], d[2], d[3]])
    far = [(600.0, 440.0 + 3 * k) for k in range(5)]
    k3 = _kf(3, 14, [_world(pa[0] + 0.5, pa[1] + 0.5), _world(pb[0] + 1, pb[1]), _world(pb[0] + 1, pb[1]), _world(*pc), (0.0, 0.0, -3.0)], far,
             [d[0], d[1], d[1], d[2], d[3]], det=[(600.0, 449.0, 20.0, 2.0, 2)])     # the box holds far[3] only: S_c is class 2
    mb, ref = _handle(), lc.new_ref()
    for kf in (k1, k2, k3):
        assert lc.add(mb, kf) == lc.add(ref, kf)
    L = ref.landmark_table()
    assert L["id"].tolist() == list(range(9)) and L["class_id"].tolist() == [0] * 7 + [2, 0] and L["observation_count"][0] == 3
    assert br.reprojection_error(ref.obs[5]["px"], L["xyz"][8], ref.kfs[1]["R"], ref.kfs[1]["t"], *ref.K) < 5, "the stand-in must be within the gate"
    want = lc.fuse(ref, 2, [3], apply=True)
    assert (want["n_sources"], want["n_targets"], want["n_proposals"], want["n_fused"]) == (5, 4, 3, 2)
    assert [p[:2] for p in want["pairs"]] == [(0, 4), (1, 5)]
    _same_fuse(mb.fuse(2, [3], apply=True), want, "special cases")
    _same_map(mb, ref, "special cases")
    assert mb.landmarks()["observation_count"][:2].tolist() == [4, 2]
    mb.close()


def test_argument_errors_leave_the_map_unchanged():
    from dvslam_amd import DvsError, PoseGraph
    mb = _handle()
    for kf in _pair_map(4, 4, seed=1):
        lc.add(mb, kf)
    before, counts = _tables(mb), mb.counts()
    pg = PoseGraph()
    nan, inf = float("nan"), float("inf")

    def refused(f, *a, **kw):
        with pytest.raises(DvsError) as e:
            f(*a, **kw)
        assert e.value.code == -6, (a, kw)

    refused(mb.fuse, 9, [1]); refused(mb.fuse, 2, [9]); refused(mb.fuse, 2, [2]); refused(mb.fuse, 2, [1, 2]); refused(mb.fuse, 2, [1, 1])
    refused(mb.fuse, 2, []); refused(mb.fuse, 2, [1] + list(range(100, 164)))
    for bad in (0.0, -1.0, nan, inf):
        refused(mb.fuse, 2, [1], max_reprojection_distance=bad); refused(mb.fuse, 2, [1], max_descriptor_distance=bad)
        refused(mb.close_loop, pg, [(2, 1, (0, 0, 0), (0, 0, 0), 1.0, 1.0)], (1.0, 1.0), fuse=dict(max_reprojection_distance=bad))
    z = (0.0, 0.0, 0.0)
    for loops, w in (([(9, 1, z, z, 1.0, 1.0)], (1.0, 1.0)), ([(2, 2, z, z, 1.0, 1.0)], (1.0, 1.0)), ([(2, 1, z, z, 0.0, 1.0)], (1.0, 1.0)),
                     ([(2, 1, z, z, 1.0, -1.0)], (1.0, 1.0)), ([(2, 1, (nan, 0, 0), z, 1.0, 1.0)], (1.0, 1.0)), ([(2, 1, z, (0, inf, 0), 1.0, 1.0)], (1.0, 1.0)),
                     ([(2, 1, z, z, 1.0, 1.0)], (0.0, 1.0)), ([(2, 1, z, z, 1.0, 1.0)], (1.0, nan))):
        refused(mb.build_pose_graph, loops, w); refused(mb.close_loop, pg, loops, w)
    assert mb.counts() == counts
    _same_tables(_tables(mb), before, "after refused calls")
    one = _handle()
    lc.add(one, _pair_map(1, 1, seed=2)[0])
    refused(one.build_pose_graph, [], (1.0, 1.0)); refused(one.close_loop, pg, [], (1.0, 1.0))
    # count-then-capacity
    n, m = C.c_int32(), C.c_int32()
    assert mb._L.dvs_backend_get_anchors(mb._h, 0, None, None, C.byref(n)) == -3 and n.value == counts["n_landmarks"]
    assert mb._L.dvs_backend_build_pose_graph(mb._h, 0, None, None, None, None, None, None, 1.0, 1.0, 0, 0, None, None, None, None, None, None, None, None, None,
                                              C.byref(n), C.byref(m)) == -3 and (n.value, m.value) == (3, 2)
    one.close(); pg.close(); mb.close()
