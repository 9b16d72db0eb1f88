"""Stage 4 of csrc/map_track.hip against tests/map_track_ref.py one Gauss-Newton step at a time, and over the sizes and the pair rules the
full-run tests leave out.  A converged run forgets how it got there: a wrong Huber weight moves the final pose of the suite's scenes by
1e-15 (tests/test_map_track_cpu.py shows it), so the test hook dvs_test_maptrack_refine_steps runs parts of the schedule and each part is
compared with the reference run on the same schedule.
Bounds.  A single step (and every schedule of STEP_SCHEDULES) is held to 10 x mr.STEP_MEASURED in every entry of R and t: STEP_MEASURED is
the float64 reference — summing by index, and in the device's lane order — against the same step in numpy.longdouble, measured on these
scenes and schedules by the CPU test; 10 is the margin the pose-graph and RANSAC stage tests give a kernel that evaluates the same
formulas with another libm.  The mutated steps of the CPU test lie more than 1000 bounds away.  Flags are compared exactly, every scene and
schedule having its gate margin asserted from the reference; the full runs keep test_gpu_map_track.py's tolerances (pose 1e-9, cost 1e-6 of
the scipy optimum, 1e-10 / 1e-9 for the whole frame).
Measured on an MI355X: the parts of the schedule 3.3e-16 .. 1.7e-15 from the reference (the bound is 2.5e-14), the full runs at 15 .. 1000
pairs 3.3e-16 .. 1.6e-15; per schedule in EXPERIMENTS.md "Map tracking"."""
import numpy as np
import pytest
import map_track_ref as mr
from test_gpu_map_track import _dev, _handle

pytestmark = pytest.mark.gpu

STEP_BOUND = 10 * mr.STEP_MEASURED


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


def _run(mt, s, schedule=None):
    """refine_device (schedule None) or the hook on scene s -> (result, inlier flags)"""
    bufs = [_dev(s["X"]), _dev(s["px"]), _dev(s["oct"].astype(np.int32))]
    if schedule is None:
        res = mt.refine_device(bufs[0], bufs[1], bufs[2], len(s["X"]), s["R0"], s["t0"])
    else:
        res = mt.refine_steps(bufs[0], bufs[1], bufs[2], len(s["X"]), s["R0"], s["t0"], *schedule)
    inl = mt.matches()[3]
    for b in bufs:
        b.free()
    return res, inl


def _ref(s, *schedule, P=None):
    return mr.refine(P or s["P"], s["R0"], s["t0"], s["X"], s["px"], s["oct"], *schedule)


def _same_bytes(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a) and set(a) == set(b)


def _dist(res, want):
    return max(float(np.abs(res["R"] - want["R"]).max()), float(np.abs(res["t"] - want["t"]).max()))


# ---------------------------------------------------------------------------------------------------- sizes
@pytest.mark.parametrize("n", [15, 63, 64, 65, 255, 256, 257, 513, 1000])
def test_refinement_sizes_around_a_wavefront_a_workgroup_and_beyond(trackers, n):
    s = mr.refine_scene(n=n, seed=7)
    want = _ref(s)
    assert want["status"] == mr.OK and mr.gate_margin(s["P"], want) > 1e-6
    mt = trackers(s["P"])
    res, inl = _run(mt, s)
    print(n, "distance", _dist(res, want), "cost", res["cost"], want["cost"])
    assert res["status"] == mr.OK and res["n_matches"] == n
    assert (inl == want["inlier"]).all() and res["n_inliers"] == want["n_inliers"]
    assert np.abs(res["R"] - want["R"]).max() < 1e-9 and np.abs(res["t"] - want["t"]).max() < 1e-9
    opt = mr.scipy_optimum(s["P"], want["Rcw"], want["tcw"], s["X"], s["px"], s["oct"], want["inlier"])
    assert abs(res["cost"] - opt) <= 1e-6 * opt, (res["cost"], opt)
    res2, inl2 = _run(mt, s)
    assert _same_bytes(res, res2) and (inl2 == inl).all()


def test_gather_over_four_chunks_of_keypoints(trackers):
    """963 keypoints, 949 kept pairs: k_mt_refine gathers them over four 256-keypoint chunks; host form and device form"""
    t = mr.track_scene(n=1000)
    want = mr.track(t["P"], t["R0"], t["t0"], t["xyz"], t["ldesc"], t["kps"], t["kdesc"])
    assert want["status"] == mr.OK and mr.gate_margin(t["P"], want) > 1e-6 and (want["inlier"] == 0).sum() > 50
    assert [int((want["kp_lm"][c:c + 256] >= 0).sum()) for c in range(0, len(t["kps"]), 256)] == [251, 254, 253, 191]
    mt = trackers(t["P"])
    bufs = [_dev(t[k]) for k in ("xyz", "ldesc", "ids", "kps", "kdesc")]
    first = None
    for form in ("host", "device"):
        if form == "host":
            res = mt.track(t["xyz"], t["ldesc"], t["ids"], t["kps"], t["kdesc"], t["R0"], t["t0"])
        else:
            res = mt.track_device(bufs[0], bufs[1], bufs[2], len(t["xyz"]), bufs[3], bufs[4], len(t["kps"]), t["R0"], t["t0"])
        row, lid, dist, inl = mt.matches()
        rec = mt.landmark_records()
        for f in mr.LM_RECORD.names:
            assert rec[f].tobytes() == want["rec"][f].tobytes(), (form, f)
        assert (row == want["kp_lm"]).all() and (dist == want["kp_dist"]).all() and (inl == want["kp_inlier"]).all()
        assert (lid == np.where(row >= 0, t["ids"][np.maximum(row, 0)], -1)).all()
        keys = ("status", "n_visible", "n_proposed", "n_matches", "n_inliers", "n_unbinned")
        assert {k: res[k] for k in keys} == {k: want[k] for k in keys}
        assert abs(res["cost"] - want["cost"]) <= 1e-9 * want["cost"]
        assert np.abs(res["R"] - want["R"]).max() < 1e-10 and np.abs(res["t"] - want["t"]).max() < 1e-10
        assert np.abs(res["t"] - t["t_true"]).max() < np.abs(t["t0"] - t["t_true"]).max()
        first = first or res
        assert _same_bytes(res, first)
    for b in bufs:
        b.free()


# ---------------------------------------------------------------------------------------------------- the stated pair rules
def test_pairs_behind_the_camera_and_outside_the_octave_table_add_nothing(trackers):
    s, behind, badoct = mr.pair_rule_scene()
    both = np.r_[behind, badoct]
    want = _ref(s)
    assert want["status"] == mr.OK and mr.gate_margin(s["P"], want) > 1e-6 and not want["inlier"][both].any() and want["n_inliers"] == 248
    res, inl = _run(trackers(s["P"]), s)
    assert res["status"] == mr.OK and (inl == want["inlier"]).all() and not inl[both].any() and res["n_inliers"] == 248
    assert np.abs(res["R"] - want["R"]).max() < 1e-9 and np.abs(res["t"] - want["t"]).max() < 1e-9
    assert abs(res["cost"] - want["cost"]) <= 1e-9 * want["cost"]
    # a table of three levels: every pair of octave >= 3 is an outlier the same way
    P3 = s["P"].with_(n_levels=3, level_sigma2=s["P"].level_sigma2[:3])
    want3 = _ref(s, P=P3)
    high = s["oct"] >= 3
    assert want3["status"] == mr.OK and mr.gate_margin(P3, want3) > 1e-6 and high.sum() > 150 and not want3["inlier"][high].any()
    res3, inl3 = _run(trackers(P3), s)
    assert res3["status"] == mr.OK and (inl3 == want3["inlier"]).all() and not inl3[high].any() and res3["n_inliers"] == want3["n_inliers"]
    assert np.abs(res3["R"] - want3["R"]).max() < 1e-9 and np.abs(res3["t"] - want3["t"]).max() < 1e-9
    assert abs(res3["cost"] - want3["cost"]) <= 1e-9 * want3["cost"]


def test_a_pair_behind_the_camera_at_the_prior_comes_in_front(trackers):
    s, i = mr.crossing_scene()
    Rp, tp = mr.pose_cw(s["R0"], s["t0"])
    want = _ref(s)
    assert mr.camera_point(Rp, tp, s["X"][i])[2] < -0.01 and want["status"] == mr.OK and want["inlier"][i] == 1 and mr.gate_margin(s["P"], want) > 1e-6
    mt = trackers(s["P"])
    res, inl = _run(mt, s)
    assert res["status"] == mr.OK and (inl == want["inlier"]).all() and inl[i] == 1 and res["n_inliers"] == want["n_inliers"]
    assert np.abs(res["R"] - want["R"]).max() < 1e-9 and np.abs(res["t"] - want["t"]).max() < 1e-9
    one_want = _ref(s, 0, 1, 1)                        # the first step skips it, the classification after it does not
    assert one_want["status"] == mr.OK and mr.gate_margin(s["P"], one_want) > 1e-6
    one, one_inl = _run(mt, s, (0, 1, 1))
    assert _dist(one, one_want) < 1e-9 and (one_inl == one_want["inlier"]).all() and one["n_inliers"] == one_want["n_inliers"]


def test_a_pixel_that_is_not_finite_ends_the_refinement(trackers):
    s = mr.refine_scene()
    for bad in (np.nan, np.inf):
        px = s["px"].copy(); px[11, 1] = bad
        d = dict(s, px=px)
        assert _ref(d)["status"] == mr.DEGENERATE
        res, inl = _run(trackers(s["P"]), d)
        assert (res["status"], res["n_matches"], res["n_inliers"], res["cost"]) == (mr.DEGENERATE, 300, 0, 0.0) and not inl.any()
        assert res["R"].tobytes() == np.ascontiguousarray(s["R0"]).tobytes() and res["t"].tobytes() == s["t0"].tobytes()


def test_a_position_that_is_not_finite_is_a_permanent_outlier(trackers):
    s = mr.refine_scene()
    rows = [11, 12, 13]
    X = s["X"].copy(); X[11, 0] = np.nan; X[12, 1] = np.inf; X[13] = -np.inf
    d = dict(s, X=X)
    want = _ref(d)
    assert _ref(s)["inlier"][rows].all() and want["status"] == mr.OK and not want["inlier"][rows].any() and mr.gate_margin(s["P"], want) > 1e-6
    res, inl = _run(trackers(s["P"]), d)
    assert res["status"] == mr.OK and (inl == want["inlier"]).all() and not inl[rows].any() and res["n_inliers"] == want["n_inliers"]
    assert np.abs(res["R"] - want["R"]).max() < 1e-9 and np.abs(res["t"] - want["t"]).max() < 1e-9
    assert abs(res["cost"] - want["cost"]) <= 1e-9 * want["cost"]


# ---------------------------------------------------------------------------------------------------- one step at a time
@pytest.fixture(scope="module")
def step_scenes():
    return mr.step_scenes()


@pytest.mark.parametrize("k", [0, 1], ids=["n300", "n257"])
@pytest.mark.parametrize("schedule", mr.STEP_SCHEDULES, ids=lambda s: "r%d_%dx%d" % s)
def test_parts_of_the_schedule_against_the_reference_on_the_same_part(trackers, step_scenes, schedule, k):
    s = step_scenes[k]
    want = _ref(s, *schedule)
    assert want["status"] == mr.OK and len(want["chi_rounds"]) == schedule[1] and mr.gate_margin(s["P"], want) > 1e-6
    mt = trackers(s["P"])
    res, inl = _run(mt, s, schedule)
    d = _dist(res, want)
    print(f"schedule {schedule} n {len(s['X'])}: distance {d:.3e} (bound {STEP_BOUND:.1e}) cost {res['cost']!r} reference {want['cost']!r}")
    assert res["status"] == mr.OK and res["n_matches"] == len(s["X"])
    assert (inl == want["inlier"]).all() and res["n_inliers"] == want["n_inliers"]
    assert abs(res["cost"] - want["cost"]) <= 1e-9 * want["cost"]
    assert STEP_BOUND <= 1e-9 and d <= STEP_BOUND
    if schedule == (0, 4, 10):                           # the product's schedule through the hook: the product's bytes
        prod, prod_inl = _run(mt, s)
        assert _same_bytes(res, prod) and (prod_inl == inl).all()


def test_the_hook_refuses_schedules_outside_the_four_rounds_of_ten(trackers, step_scenes):
    from dvslam_amd._lib import DvsError
    s = step_scenes[1]
    mt = trackers(s["P"])
    for bad in [(-1, 1, 1), (0, 0, 1), (0, 5, 1), (3, 2, 1), (4, 1, 1), (0, 1, 0), (0, 1, 11), (2147483647, 2147483647, 1)]:
        with pytest.raises(DvsError) as e:
            _run(mt, s, bad)
        assert e.value.code == -6, bad
    res, _ = _run(mt, dict(s, X=s["X"][:14], px=s["px"][:14], oct=s["oct"][:14]), (3, 1, 10))
    assert res["status"] == mr.FEW_MATCHES and res["R"].tobytes() == np.ascontiguousarray(s["R0"]).tobytes()
