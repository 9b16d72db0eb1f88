"""dvs_tracker_* on the GPU (csrc/tracker.hip): one call per RGB-D frame against the same frame loop over the library's one-stage
host-pointer entry points (tests/tracker_ref.py over tools/replay_tracking.py's HipStages — same kernels, same inputs, so everything is
required bit for bit), against the CPU oracle pipeline (bars of tests/test_tracking_replay.py: identical keyframes, <= 3 mm / 0.1 deg
RMS over 60 frames), on the edge frames of Frontend::syncCallback, with OpenCV's procedures in both RANSAC stages, and through the C++
adapter.  No wall-clock assertion (tools/track_sequence.py measures)."""
import os
import subprocess
import sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIBDIR = os.path.join(ROOT, "dynamic-visual-slam_amd", "lib")
COLS, ROWS, F, Z0, NF = 640, 480, 600.0, 1.5, 1000
CX, CY = COLS / 2.0, ROWS / 2.0


def _tracker(**kw):
    from dvslam_amd import tracker as T
    return T.Tracker(T.default_params(ROWS, COLS, F, F, CX, CY, nfeatures=NF, **kw))


def _frames(ts, seed=1234):
    from dvslam_amd import synth
    return [synth.make_traj_frame(t, COLS, ROWS, seed=seed) for t in ts]


def _flat(n, mm=1500):
    return [np.full((ROWS, COLS), mm, np.uint16) for _ in range(n)]


def _relief(n, mm=200):
    d = np.full((ROWS, COLS), 1500, np.uint16)
    yy, xx = np.mgrid[0:ROWS, 0:COLS]
    d[((yy // 64 + xx // 64) & 1) == 1] += np.uint16(mm)
    return [d.copy() for _ in range(n)]


def _poses(run):
    return [(r["R"], r["t"]) for r in run]


def test_sixty_frames_equal_the_one_stage_entry_points_bit_for_bit(gpu, hooks):
    """own estimators, seed base 0: every count, flag, keyframe id, culled selection, rvec / tvec, CDR payload and R_ / t_"""
    import replay_tracking as rt
    import tracker_ref as ref
    frames, depths = _frames(range(60)), _flat(60)
    want = ref.track_ref(rt.HipStages(NF), hooks, frames, depths, F, CX, CY, fm_mode=0, pnp_mode=0, seed_base=0)
    tr = _tracker()
    got = ref.run_tracker(tr, frames, depths)
    assert ref.first_difference(got, want) is None, ref.first_difference(got, want)
    assert sum(r["pose_updated"] for r in got) == 59 and sum(r["is_keyframe"] for r in got) >= 2 and got[1]["kf_criterion"] == 2
    assert min(r["n_geometric"] for r in got[1:]) > 300 and all(r["payload"] for r in got if r["is_keyframe"])
    # reset() and the same sequence again: the same results
    tr.reset()
    again = ref.run_tracker(tr, frames[:12], depths[:12])
    assert ref.first_difference(again, got[:12]) is None, ref.first_difference(again, got[:12])
    # another seed base draws other samples: the seed schedule is live
    other = ref.run_tracker(_tracker(seed_base=77), frames[:4], depths[:4])
    assert any(a["rvec"].tobytes() != b["rvec"].tobytes() for a, b in zip(other[1:], got[1:4]))
    tr.close()


def test_sixty_frames_against_the_cpu_oracle_pipeline(gpu, oracle, hooks):
    """the existing 60-frame replay's configuration (OpenCV's procedure in the fundamental-matrix gates, P3P + LM with the shared sampler in
    the pose stage) and its bars: identical keyframes, <= 3 mm / 0.1 deg RMS"""
    import replay_tracking as rt
    import tracker_ref as ref
    frames, depths = _frames(range(60)), _flat(60)
    cpu = ref.track_ref(rt.CpuStages(NF), hooks, frames, depths, F, CX, CY, fm_mode=1, pnp_mode=0, seed_base=0)
    tr = _tracker(fm_mode=1)
    got = ref.run_tracker(tr, frames, depths)
    tr.close()
    assert [r["is_keyframe"] for r in got] == [r["is_keyframe"] for r in cpu] and sum(r["is_keyframe"] for r in got) >= 2
    assert [r["n_matches"] for r in got] == [r["n_matches"] for r in cpu]          # extraction / match / glue are bit-exact
    e = rt.rmse(_poses(got), _poses(cpu))
    print("tracker vs CPU oracle pipeline:", e)
    assert e["translation_m"] < 3e-3 and e["rotation_deg"] < 0.1, e
    g = rt.rmse(_poses(got), rt.ground_truth(60, F, Z0))
    assert g["translation_m"] < 0.06 and g["rotation_deg"] < 2.5, g


def test_edge_frames(gpu, hooks):
    """reset and recovery (blank image, all-zero depth), fewer than 8 matches, a jump past the motion gate: the branches of
    syncCallback, each reached and each equal to the one-stage loop"""
    import replay_tracking as rt
    import tracker_ref as ref
    base = _frames(range(12))
    frames = list(base); depths = _flat(12)
    frames[4] = np.zeros((ROWS, COLS), np.uint8)                    # blank: no features -> reset; frame 5 finds prev_kps_ empty -> reset; 6 tracks
    depths[8] = np.zeros((ROWS, COLS), np.uint16)                   # no feature survives filterDepth -> reset, and again at 9
    depths[11] = np.zeros((ROWS, COLS), np.uint16); depths[11][220:260, 300:340] = 1500   # depth in a 40 x 40 window only: 5 features survive, so < 8 matches
    want = ref.track_ref(rt.HipStages(NF), hooks, frames, depths, F, CX, CY)
    tr = _tracker()
    got = ref.run_tracker(tr, frames, depths)
    assert ref.first_difference(got, want) is None, ref.first_difference(got, want)
    assert [r["tracking_reset"] for r in got] == [0, 0, 0, 0, 1, 1, 0, 0, 1, 1, 0, 0]
    assert got[4]["n_extracted"] == 0 and got[8]["n_extracted"] > 500 and got[8]["n_filtered"] == 0
    assert got[6]["pose_updated"] == 1 and got[10]["pose_updated"] == 1 and not any(r["is_keyframe"] for r in got[4:6])
    print("windowed frame:", got[11]["n_filtered"], "features,", got[11]["n_matches"], "matches,", got[11]["n_pnp_points"], "PnP points")
    assert 0 < got[11]["n_filtered"] < 8 and got[11]["n_matches"] < 8 and got[11]["fm_skipped"] == 1 and got[11]["n_geometric"] == got[11]["n_matches"]
    assert got[11]["pnp_skipped"] == 1 and got[11]["pose_updated"] == 0                # fewer than 6 points can come of it
    assert (got[5]["R"] == got[3]["R"]).all() and (got[5]["t"] == got[3]["t"]).all()
    tr.close()
    # a jump of ~116 px at 2.95 m is ~0.57 m between two frames: PnP succeeds, isMotionOutlier rejects it (0.5 m)
    ts = [0, 1, 2, 3, 33, 34]
    frames, depths = _frames(ts), _flat(len(ts), 2950)
    want = ref.track_ref(rt.HipStages(NF), hooks, frames, depths, F, CX, CY)
    tr = _tracker()
    got = ref.run_tracker(tr, frames, depths)
    tr.close()
    assert ref.first_difference(got, want) is None, ref.first_difference(got, want)
    print("jump frame:", {k: got[4][k] for k in ("n_matches", "n_geometric", "n_pnp_points", "n_pnp_inliers", "motion_outlier")}, got[4]["tvec"])
    assert got[4]["motion_outlier"] == 1 and got[4]["pose_updated"] == 0 and got[4]["n_pnp_inliers"] > 0
    assert (got[4]["t"] == got[3]["t"]).all() and got[5]["pose_updated"] == 1


def test_static_frames_reach_the_thirty_frame_rule(gpu, hooks):
    """a camera that stays put (views 10, 11, then 12 and 10 in turn: never the keyframe's own image, whose identical points make the
    fundamental matrix degenerate): frame 0 is the first keyframe, frame 1 the first isKeyframe call (no reference yet), then
    frames_since_last_keyframe_ counts 31 frames up and the > 30 rule fires at frame 33"""
    import replay_tracking as rt
    import tracker_ref as ref
    frames, depths = _frames([10, 11] + [12, 10] * 17), _flat(36)
    want = ref.track_ref(rt.HipStages(NF), hooks, frames, depths, F, CX, CY)
    tr = _tracker()
    got = ref.run_tracker(tr, frames, depths)
    tr.close()
    assert ref.first_difference(got, want) is None, ref.first_difference(got, want)
    assert [t for t, r in enumerate(got) if r["is_keyframe"]] == [0, 1, 33]
    assert got[33]["kf_criterion"] == 8 and got[33]["keyframe_id"] == 2 and got[34]["is_keyframe"] == 0 and min(r["n_kf_geometric"] for r in got[2:33]) >= 150


def test_three_channel_input_equals_the_gray_path(gpu, hooks):
    import tracker_ref as ref
    from dvslam_amd import FrontendGlue
    g = FrontendGlue()
    a = _frames(range(6)); b = _frames(range(6), seed=7)
    bgr = [np.ascontiguousarray(np.stack([a[t], b[t], np.roll(a[t], 9, axis=1)], 2)) for t in range(6)]
    gray = [g.bgr_to_gray(x, 0) for x in bgr]
    depths = _flat(6)
    t3, t1 = _tracker(), _tracker()
    got3, got1 = ref.run_tracker(t3, bgr, depths), ref.run_tracker(t1, gray, depths)
    t3.close(); t1.close()
    assert ref.first_difference(got3, got1) is None, ref.first_difference(got3, got1)
    assert got3[5]["n_extracted"] > 500 and got3[5]["pose_updated"] == 1


def _padded(a, extra, fill):
    """the same pixels as rows of a wider buffer: strides[0] larger than the row, and `fill` in the padding"""
    buf = np.full((a.shape[0], a.shape[1] + extra) + a.shape[2:], fill, a.dtype)
    buf[:, :a.shape[1]] = a
    view = buf[:, :a.shape[1]]
    assert view.strides[0] > a.shape[1] * a.itemsize * (a.shape[2] if a.ndim == 3 else 1) and not view.flags["C_CONTIGUOUS"]
    return view


def test_row_padded_input_equals_the_contiguous_run(gpu, hooks):
    """image.strides[0] and depth.strides[0] larger than the row (the row-by-row staging of dvs_tracker_track) over ten frames, gray and
    BGR: everything equal to the contiguous run, R_ / t_ bit for bit.  The relief depth makes a wrong depth row show in filterDepth's
    survivors and in the PnP points; the padding holds values no frame has."""
    import tracker_ref as ref
    a = _frames(range(10)); depths = _relief(10)
    bgr = [np.ascontiguousarray(np.stack([x, np.roll(x, 5, axis=0), np.roll(x, 9, axis=1)], 2)) for x in a]
    for frames in (a, bgr):
        tc, tp = _tracker(), _tracker()
        want = ref.run_tracker(tc, frames, depths)
        got = ref.run_tracker(tp, [_padded(x, 24, 255) for x in frames], [_padded(d, 8, 65535) for d in depths])
        tc.close(); tp.close()
        assert ref.first_difference(got, want, poses_bitwise=True) is None, ref.first_difference(got, want, poses_bitwise=True)
        assert want[9]["n_extracted"] > 500 and sum(r["pose_updated"] for r in want) >= 5      # the runs are not trivially equal


def test_opencv_procedures_on_the_relief_scene(gpu, hooks):
    """fm_mode = pnp_mode = 1 (dvs_find_fundamental_cv / dvs_solve_pnp_ransac_cv) on the scene with a 200 mm depth relief, against the same
    loop over the host-pointer _cv entry points: the same equality as with the own estimators"""
    import replay_tracking as rt
    import tracker_ref as ref
    frames, depths = _frames(range(30)), _relief(30)
    want = ref.track_ref(rt.HipStages(NF), hooks, frames, depths, F, CX, CY, fm_mode=1, pnp_mode=1)
    tr = _tracker(fm_mode=1, pnp_mode=1)
    got = ref.run_tracker(tr, frames, depths)
    tr.close()
    assert ref.first_difference(got, want) is None, ref.first_difference(got, want)
    assert sum(r["pose_updated"] for r in got) == 29 and rt.PNP_MODE == "own"


def test_cdr_capacity_overflow_reports_the_needed_size(gpu):
    import ctypes as C
    from dvslam_amd import tracker as T, DvsError
    tr = _tracker()
    img, depth = _frames([0])[0], _flat(1)[0]
    r = T.TrackResult(); small = np.zeros(64, np.uint8)
    code = tr._L.dvs_tracker_track(tr._h, img.ctypes.data, 1, COLS, depth.ctypes.data, COLS * 2, 0, 0, C.byref(r), small.ctypes.data, 64)
    assert code == -3 and r.is_keyframe == 1 and r.cdr_bytes > 64 and r.n_filtered > 500
    with pytest.raises(ValueError):
        tr.track(img[:100], depth)
    assert DvsError is not None
    tr.close()


def test_cpp_adapter_program_equals_the_python_mirror(gpu, tmp_path):
    """tests/cpp/tracker_adapter.cpp (dvslam::TrackingFrontend) over 20 frames written to a file, printed as text, against the mirror"""
    import tracker_ref as ref
    exe = os.path.join(str(tmp_path), "tracker_adapter")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "tracker_adapter.cpp"), "-o", exe, "-L" + LIBDIR, "-ldvslam_hip", "-Wl,-rpath," + LIBDIR,
                           "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    frames, depths = _frames(range(20)), _flat(20)
    path = os.path.join(str(tmp_path), "frames.bin")
    with open(path, "wb") as fh:
        for a in frames:
            fh.write(a.tobytes())
    out = subprocess.run([exe, path, str(ROWS), str(COLS), "20", str(F), "1500"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    tr = _tracker()
    got = ref.run_tracker(tr, frames, depths)
    tr.close()
    import zlib
    lines = []
    for r in got:
        pose = " ".join(format(int(np.float64(v).view(np.uint64)), "016x") for v in list(r["R"].ravel()) + list(r["t"]))
        lines.append(f"{r['frame_index']} kf={r['is_keyframe']} id={r['keyframe_id']} crit={r['kf_criterion']} n={r['n_extracted']},{r['n_filtered']},{r['n_matches']},"
                     f"{r['n_geometric']},{r['n_pnp_points']},{r['n_pnp_inliers']},{r['n_backend']} upd={r['pose_updated']} cdr={len(r['payload'] or b'')},"
                     f"{zlib.crc32(r['payload'] or b'')} pose={pose}")
    assert out.stdout.strip().splitlines() == lines


def _cull_device(hooks, response, matched, max_new=200, min_response=50.0):
    import ctypes as C
    response = np.ascontiguousarray(response, np.float32); matched = np.ascontiguousarray(matched, np.uint8)
    n = len(response)
    order = np.zeros(max(n, 1), np.int32); m = C.c_int32(); heaps = C.c_int32()
    hooks.dvs_test_cull_order_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    code = hooks.dvs_test_cull_order_device(response.ctypes.data, matched.ctypes.data, n, max_new, min_response, order.ctypes.data, C.byref(m), C.byref(heaps))
    assert code == 0, hooks.dvs_last_error()
    return order[:m.value].astype(np.int64), heaps.value


def test_culling_kernel_orders_like_the_host_hook_on_tie_heavy_vectors(gpu, hooks):
    """k_cull's own sort driver (explicit stack, leaves placed by rank, heapsort at the depth limit) on the CPU suite's vectors — which
    tests/test_tracker_cull_order.py holds against the real std::sort through the host hook — and on two inputs built against the
    median-of-3 pivot, on which the introsort must reach its depth limit: index-for-index equality, and the heapsort branch is taken"""
    import test_tracker_cull_order as cc
    import tracker_ref as ref
    n_cases = 0
    for name, resp, matched in cc._cases():
        got, _ = _cull_device(hooks, resp, matched)
        want = ref.cull_order(hooks, resp, matched)
        assert len(got) == len(want) and (got == want).all(), name
        n_cases += 1
    assert n_cases == 42
    heap_total = 0
    for n in (700, 1024, 2000):
        k = n // 2
        musser = np.array([(i + 1 if i % 2 == 0 else k + i) for i in range(k)] + [2 * (i + 1) for i in range(k)], np.int64)
        pipe = np.concatenate([np.arange(1, k + 1, 2), np.arange(k + 1, n + 1), np.arange(2, k + 1, 2)])
        pipe = np.concatenate([pipe, np.ones(n - len(pipe), np.int64)])[:n]
        for v in (musser, pipe):
            resp = (4096 - v).astype(np.float32)                      # the comparator sorts descending: ascending v
            matched = np.zeros(len(resp), np.uint8)
            got, heaps = _cull_device(hooks, resp, matched, max_new=len(resp), min_response=0.0)
            want = ref.cull_order(hooks, resp, matched, len(resp), 0.0)
            assert len(got) == len(resp) and (got == want).all() and heaps >= 1, (n, heaps)
            heap_total += heaps
    print("ranges sorted by the heapsort branch:", heap_total)


pytestmark = pytest.mark.gpu
