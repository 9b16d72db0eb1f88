"""Stages 1-3 of csrc/map_track.hip bit for bit against tests/map_track_ref.py at the structure of a real frame: test_gpu_map_track.py's
check_search (every field of every record, the CSR, the matches, the counts) on scenes where the per-keypoint kernels run as several
workgroups, k_mt_scan carries its base over several 256-cell chunks, one cell's segment is longer than a workgroup and straddles two of
k_mt_order's, many workgroups of landmarks propose to few keypoints, one handle serves a big, a small and a big call, and the handle works
on a stream of its own without waiting.  That each scene really has the property it is here for is asserted from the reference — here, and
without a GPU in tests/test_map_track_cpu.py."""
import numpy as np
import pytest
import map_track_ref as mr
from test_gpu_map_track import check_search, _dev, _handle, trackers   # noqa: F401  (trackers: the module-scoped fixture)

pytestmark = pytest.mark.gpu

PF = mr.frame_params()
R, T = mr.FRAME_R, mr.FRAME_T


@pytest.mark.parametrize("n_lm,n_kp", [(1000, 255), (1000, 256), (1000, 257), (1000, 513), (3000, 2000)])
def test_keypoint_counts_around_a_workgroup_and_a_whole_frame(trackers, n_lm, n_kp):   # noqa: F811
    xyz, ld, kps, kd, ids = mr.frame_scene(PF, n_lm, n_kp)
    want, lm, _ = check_search(trackers(PF), PF, xyz, ld, kps, kd, R, T, ids)
    assert want["proposed"].sum() > 100 and (lm >= 0).sum() > 100
    if n_kp == 2000:
        assert (lm >= 0).sum() < want["proposed"].sum() - 100            # landmarks lost their keypoint to another


def _chunks(P, kps):
    start, _, _ = mr.bin_keypoints(P, kps)
    n = len(start) - 1
    return [int(start[min(c + 256, n)] - start[c]) for c in range(0, n, 256)]


@pytest.mark.parametrize("rows,cols,cell,ncell", [(512, 512, 32, 256), (1, 257, 1, 257), (480, 640, 32, 300), (480, 640, 16, 1200)])
def test_grids_of_one_scan_chunk_one_cell_more_and_five_chunks(trackers, rows, cols, cell, ncell):   # noqa: F811
    P = PF.with_(rows=rows, cols=cols, cell=cell)
    xyz, ld, kps, kd, ids = mr.frame_scene(P, 1000, 513)
    chunks = _chunks(P, kps)
    assert len(chunks) == (ncell + 255) // 256 and min(chunks) > 0 and sum(chunks) == 513      # every chunk holds keypoints, the last included
    check_search(trackers(P), P, xyz, ld, kps, kd, R, T, ids)


def test_outcome_at_640_x_480_does_not_depend_on_the_cell_size(trackers):   # noqa: F811
    xyz, ld, kps, kd, ids = mr.frame_scene(PF, 1000, 513)
    a, lm_a, d_a = check_search(trackers(PF), PF, xyz, ld, kps, kd, R, T, ids)
    for cell in (16, 8):
        Pc = PF.with_(cell=cell)
        assert min(_chunks(Pc, kps)) > 0
        b, lm_b, d_b = check_search(trackers(Pc), Pc, xyz, ld, kps, kd, R, T, ids)
        assert a.tobytes() == b.tobytes() and (lm_a == lm_b).all() and (d_a == d_b).all()


@pytest.mark.parametrize("n_before", [0, 200])
def test_a_cell_of_more_than_one_workgroup(trackers, n_before):   # noqa: F811
    """300 keypoints in one cell: its segment of the CSR is ranked by more than one workgroup of k_mt_order, from slot 0 and from slot 200
    (over the boundary between slots 255 and 256); arrival order is not index order"""
    P = mr.small_params()
    xyz, ld, kps, kd, cell = mr.dense_cell_scene(P, n_before)
    start, order, _ = mr.bin_keypoints(P, kps)
    assert (start[cell], start[cell + 1]) == (n_before, n_before + 300) and (order != np.arange(len(order))).any()
    want, lm, _ = check_search(trackers(P), P, xyz, ld, kps, kd)
    assert (want["d_second"] >= 0).sum() > 50 and (lm >= 0).sum() > 10


def test_many_workgroups_of_landmarks_propose_to_few_keypoints(trackers):   # noqa: F811
    """20000 landmarks in 79 workgroups, 2000 keypoints: the 64-bit atomicMin decides between up to ten proposals per keypoint"""
    xyz, ld, kps, kd, ids = mr.crowded_scene(PF)
    Rcw, tcw = mr.pose_cw(R, T)
    rec = mr.search_grid(PF, Rcw, tcw, xyz, ld, kps, kd)
    lm, _ = mr.assign(rec, len(kps))
    n = mr.proposals_per_keypoint(rec, len(kps))
    assert (lm >= 0).sum() > 1000 and 2 * (n[lm >= 0] >= 2).sum() >= (lm >= 0).sum()
    check_search(trackers(PF), PF, xyz, ld, kps, kd, R, T, ids)


def _getters(mt):
    return [a.tobytes() for a in (mt.landmark_records(),) + mt.cells() + mt.matches()]


def test_one_handle_big_then_small_then_big(gpu):
    """a handle of its own, so that its buffers grow with the first call; the small calls must show nothing of the big one (check_search
    compares every row and every cell the getters return), also after a refinement has used the per-keypoint buffers"""
    big, small = mr.frame_scene(PF, 3000, 2000), mr.frame_scene(PF, 65, 40)
    s = mr.refine_scene(n=1000, seed=7)
    mt = _handle(PF)
    try:
        first = None
        for scene in (big, small, big):
            xyz, ld, kps, kd, ids = scene
            check_search(mt, PF, xyz, ld, kps, kd, R, T, ids)
            if scene is big:
                got = _getters(mt)
                assert first is None or got == first                 # identical bytes in every getter
                first = got
        bufs = [_dev(s["X"]), _dev(s["px"]), _dev(s["oct"].astype(np.int32))]
        res = mt.refine_device(bufs[0], bufs[1], bufs[2], 1000, s["R0"], s["t0"])
        assert res["status"] == mr.OK and res["n_matches"] == 1000 and len(mt.matches()[0]) == 1000 and len(mt.landmark_records()) == 0
        for b in bufs:
            b.free()
        xyz, ld, kps, kd, ids = small
        check_search(mt, PF, xyz, ld, kps, kd, R, T, ids)
    finally:
        mt.close()


def test_a_stream_of_its_own_and_the_search_that_does_not_wait(gpu):
    from dvslam_amd._lib import stream_create, stream_destroy
    xyz, ld, kps, kd, ids = mr.frame_scene(PF, 1000, 513)
    Rcw, tcw = mr.pose_cw(R, T)
    want = mr.search_grid(PF, Rcw, tcw, xyz, ld, kps, kd)
    lm, d = mr.assign(want, len(kps))
    wstart, worder, _ = mr.bin_keypoints(PF, kps)
    t = mr.track_scene()
    twant = mr.track(t["P"], t["R0"], t["t0"], t["xyz"], t["ldesc"], t["kps"], t["kdesc"])
    assert twant["status"] == mr.OK and mr.gate_margin(t["P"], twant) > 1e-6 and t["P"].__dict__ == PF.__dict__
    stream = stream_create()
    mt = _handle(PF)
    try:
        mt.set_stream(stream)
        bufs = [_dev(xyz), _dev(ld), _dev(ids), _dev(kps), _dev(kd)]
        assert mt.search_device(bufs[0], bufs[1], bufs[2], 1000, bufs[3], bufs[4], 513, R, T, want_counts=False) is None
        row, lid, dist, inl = mt.matches()                           # the getters wait on the handle's stream
        rec = mt.landmark_records(); start, order = mt.cells()
        for f in mr.LM_RECORD.names:
            assert rec[f].tobytes() == want[f].tobytes(), f
        assert (start == wstart).all() and (order == worder).all()
        assert (row == lm).all() and (dist == d).all() and not inl.any() and (lid == np.where(lm >= 0, ids[np.maximum(lm, 0)], -1)).all()
        for b in bufs:
            b.free()
        # stages 1-4 on the same stream
        bufs = [_dev(t["xyz"]), _dev(t["ldesc"]), _dev(t["ids"]), _dev(t["kps"]), _dev(t["kdesc"])]
        res = mt.track_device(bufs[0], bufs[1], bufs[2], len(t["xyz"]), bufs[3], bufs[4], len(t["kps"]), t["R0"], t["t0"])
        row, lid, dist, inl = mt.matches()
        rec = mt.landmark_records()
        for f in mr.LM_RECORD.names:
            assert rec[f].tobytes() == twant["rec"][f].tobytes(), f
        assert (row == twant["kp_lm"]).all() and (dist == twant["kp_dist"]).all() and (inl == twant["kp_inlier"]).all()
        keys = ("status", "n_visible", "n_proposed", "n_matches", "n_inliers", "n_unbinned")
        assert {k: res[k] for k in keys} == {k: twant[k] for k in keys}
        assert abs(res["cost"] - twant["cost"]) <= 1e-9 * twant["cost"]
        assert np.abs(res["R"] - twant["R"]).max() < 1e-10 and np.abs(res["t"] - twant["t"]).max() < 1e-10
        for b in bufs:
            b.free()
        mt.set_stream(None)
    finally:
        mt.close()
        stream_destroy(stream)
