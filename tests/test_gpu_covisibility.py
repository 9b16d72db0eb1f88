"""GPU: the covisibility graph, the local BA window, local BA and tracking against the local map (include/dvslam_hip.h "Covisibility")
against the restatement over the handle's own getters (tests/covisibility_ref.py), bit for bit.  The scenes' conditions are asserted without
a GPU in tests/test_covisibility_cpu.py; the few that decide whether a test here checks anything are asserted again on the device's tables."""
import numpy as np
import pytest
import backend_ref as br
import covisibility_ref as cr
import loop_closing_ref as lc

pytestmark = pytest.mark.gpu
TABLE_KEYS = ("landmarks", "observations", "keyframes")


def _handle(keyframes):
    from dvslam_amd.backend import MappingBackend
    mb = MappingBackend(br.FX, br.FY, br.CX, br.CY, filtered=("person",), initial_capacity=64)
    assert mb.intern("person") == br.PERSON and mb.intern("chair") == br.CHAIR and mb.intern("table") == br.TABLE
    for kf in keyframes:
        lc.add(mb, kf)
    return mb


def _fused_handle():
    mb = _handle(br.make_scene())
    out = mb.fuse(cr.FUSED_QUERY, cr.FUSED_ENTRIES, **cr.FUSED_PARAMS)
    assert out["n_fused"] > 0
    return mb


def _tables(mb):
    return mb.landmarks(), mb.observations(), mb.keyframes()


def _same_bytes(a, b):
    for x, y in zip(a, b):
        assert set(x) == set(y)
        for k in x:
            assert np.asarray(x[k]).tobytes() == np.asarray(y[k]).tobytes(), k


def _same_dict(got, want, what):
    for k in got:
        if isinstance(got[k], np.ndarray):
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), (what, k)
        else:
            assert got[k] == want[k], (what, k)


class Scene:
    """a handle, its tables as the getters return them (read once: every call under test is read-only) and the restatement's sets"""

    def __init__(self, mb):
        self.mb = mb
        self.before = _tables(mb)
        lms, obs, kfs = self.before
        self.T = (kfs, lms, obs)
        self.S = cr.observes(*self.T)
        self.W = cr.weights(self.S)
        self.frames = [int(f) for f in kfs["frame_id"]]

    def window(self, frame, **params):
        return cr.local_window(*self.T, frame, (self.S, self.W), **params)

    def unchanged(self):
        _same_bytes(_tables(self.mb), self.before)


SCENES = {"hub": lambda: _handle(cr.hub_scene()), "fused": _fused_handle, "one": lambda: _handle(br.make_scene()[:1]), "two": lambda: _handle(br.make_scene()[:2])}


@pytest.fixture(scope="module")
def scenes(gpu):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Scene(SCENES[name]())
        return made[name]
    yield get
    for s in made.values():
        s.mb.close()


@pytest.mark.parametrize("name", list(SCENES))
def test_graph_equals_the_restatement(scenes, name):
    """fails without the feature (no MappingBackend.covisibility)"""
    s = scenes(name)
    got = {}
    for theta in (1, 15):
        got[theta] = s.mb.covisibility(theta)
        want = cr.graph(*s.T, theta)
        _same_dict(got[theta], want, (name, theta))
        again = s.mb.covisibility(theta)
        _same_dict(again, got[theta], (name, theta, "second call"))
        lists_only = s.mb.covisibility(theta, weights=False)
        assert lists_only["weights"] is None and lists_only["nb_index"].tobytes() == want["nb_index"].tobytes()
    if name == "hub":
        cr.hub_conditions(got[1], got[15])                                   # the device's association followed the designed incidence
    if name == "fused":
        assert cr.repeated_pairs(*s.T) > 0                                    # a keyframe names a landmark twice, and counts it once
    s.unchanged()


def _refs(name, s):
    if name == "hub":
        return [cr.HUB_FRAME0 + cr.HUB, cr.HUB_FRAME0 + cr.HUB_LEAF, s.frames[0], s.frames[-1]]
    return sorted(set([s.frames[0], s.frames[len(s.frames) // 2], s.frames[-1]]))


@pytest.mark.parametrize("name", list(SCENES))
def test_local_window_equals_the_restatement(scenes, name):
    s = scenes(name)
    thetas = (15, 1) if name == "hub" else (15,)
    left, gauge, fixed = [], 0, 0
    for theta in thetas:
        for frame in _refs(name, s):
            for mn in (0, 3, 10):
                for mf in (0, 2, 32):
                    params = dict(min_weight=theta, max_neighbours=mn, max_fixed=mf)
                    got = s.mb.local_window(frame, **params)
                    want = s.window(frame, **params)
                    want.pop("kf_index")
                    _same_dict(got, want, (name, frame, params))
                    assert (got["obs_lm_index"] >= 0).all() and got["kf_fixed"].sum() >= 1
                    left.append(got["n_left_out"])
                    free = got["kf_fixed"] == 0
                    gauge += int(mf == 0 and got["kf_fixed"].sum() == 1 and free.sum() == min(mn, len(s.frames) - 1))    # a free keyframe became the gauge
                    fixed += int(got["kf_fixed"].sum() == mf and mf > 0 and free.sum() == mn + 1)
    got = s.mb.local_window(s.frames[-1])
    _same_dict(s.mb.local_window(s.frames[-1]), got, (name, "second call"))
    if name == "hub":
        assert fixed > 0 and gauge > 0                                        # full lists of both kinds, and the gauge
    if name == "fused":
        assert max(left) > 0 and gauge > 0
    s.unchanged()


def _solve_directly(window):
    """the restatement's problem through dvs_ba_set_problem + dvs_ba_solve_device -> (summary, problem, used, dropped, parameters)"""
    from dvslam_amd import BAProblem
    P, used, dropped = cr.local_ba_problem(window, br.FX, br.FY, br.CX, br.CY)
    g = BAProblem(P)
    return g, P, used, dropped


@pytest.mark.parametrize("fused", [False, True], ids=["plain", "fused"])
def test_local_bundle_adjust_equals_the_same_problem_solved_directly(gpu, fused):
    import global_ba_ref as gr
    make = _fused_handle if fused else (lambda: _handle(br.make_scene()))
    mb, other = make(), make()
    before = _tables(mb)
    lms, obs, kfs = before
    _same_bytes(_tables(other), before)
    frame = int(kfs["frame_id"][-1])
    w = cr.local_window(kfs, lms, obs, frame)
    g, P, used, dropped = _solve_directly(w)
    n_free = int((w["kf_fixed"] == 0).sum())
    assert 2 <= n_free <= 16 and used.sum() > 50 and (not fused or max(cr.local_window(kfs, lms, obs, f)["n_left_out"] for f in (frame, int(kfs["frame_id"][0]))) > 0)

    # a solve that does not converge leaves every byte of the map
    capped = mb.local_bundle_adjust(frame, ba_max_iterations=1)
    assert capped["summary"].termination == 1 and capped["summary"].num_iterations == 1
    _same_bytes(_tables(mb), before)

    out = mb.local_bundle_adjust(frame)
    s = out["summary"]
    sg = g.solve_device(20, 1e-6, 1e-10, 1e-8)
    print(f"local BA at frame {frame}: {P['K']} cameras ({n_free} free), {P['L']} landmarks, {len(P['cam_idx'])} observations, {dropped} dropped, "
          f"{w['n_left_out']} left out; cost {s.initial_cost!r} -> {s.final_cost!r}, termination {s.termination}, {s.num_iterations} iterations")
    assert {k: out[k] for k in out if k != "summary"} == dict(n_cameras=P["K"], n_fixed=int(w["kf_fixed"].sum()), n_landmarks=P["L"],
                                                              n_observations=len(P["cam_idx"]), n_left_out=w["n_left_out"], n_dropped=dropped)
    assert (s.termination, s.num_successful_steps, s.num_iterations, s.linear_solver, s.initial_cost, s.final_cost) == \
        (sg.termination, sg.num_successful_steps, sg.num_iterations, sg.linear_solver, sg.initial_cost, sg.final_cost)
    assert s.linear_solver == 1 and s.termination == 0 and s.final_cost <= s.initial_cost
    # the second backend, fed the same scene, gets the direct solve's parameters through apply_optimized
    q, t, X = g.parameters()
    poses = {int(w["kf_frame_id"][k]): gr.pose_to_rt(q[k], t[k]) for k in range(P["K"]) if not w["kf_fixed"][k]}
    positions = {(int(i), int(c)): X[j] for j, (i, c) in enumerate(zip(w["lm_id"][used], w["lm_class"][used]))}
    other.apply_optimized(poses, positions)
    after = _tables(mb)
    _same_bytes(after, _tables(other))
    # what is outside the problem kept its bytes, what is inside moved
    lms2, _, kfs2 = after
    inside = np.isin(kfs["frame_id"], w["kf_frame_id"][w["kf_fixed"] == 0])
    assert kfs2["R"][~inside].tobytes() == kfs["R"][~inside].tobytes() and kfs2["t"][~inside].tobytes() == kfs["t"][~inside].tobytes()
    assert all(kfs2["R"][k].tobytes() != kfs["R"][k].tobytes() for k in np.nonzero(inside)[0])
    in_problem = np.isin(lms["id"], w["lm_id"][used])
    assert (~in_problem).any() and lms2["xyz"][~in_problem].tobytes() == lms["xyz"][~in_problem].tobytes()
    assert (lms2["xyz"][in_problem] != lms["xyz"][in_problem]).any()
    for a, b in zip(before, after):
        for k in a:
            if k not in ("xyz", "R", "t"):
                assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k
    mb.close(); other.close()


def _frame_of(kf, rng):
    """the keypoints a keyframe of make_scene() would give the tracker: its pixels in another order, five bits of every descriptor flipped"""
    import map_track_ref as mr
    n = len(kf["px"])
    perm = rng.permutation(n)
    kps = mr.keypoints(kf["px"][perm].astype(np.float32))
    kps["octave"] = rng.integers(0, 3, n)
    kd = kf["desc"][perm].copy()
    for k in range(n):
        for b in rng.choice(256, 5, replace=False):
            kd[k, b >> 3] ^= np.uint8(1 << (b & 7))
    return kps, kd


def _track_equal(res, mt, want, mt2):
    for k in res:
        if isinstance(res[k], np.ndarray):
            assert res[k].tobytes() == want[k].tobytes(), k
        else:
            assert res[k] == want[k] or (k == "cost" and np.float64(res[k]).tobytes() == np.float64(want[k]).tobytes()), k
    for a, b in zip(mt.matches(), mt2.matches()):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_track_frame_local_equals_the_tracker_on_the_restatements_local_map(scenes):
    from dvslam_amd import map_track as M
    from dvslam_amd._lib import DeviceBuffer
    import map_track_ref as mr
    s = scenes("fused")
    kf = br.make_scene()[-1]
    kps, kd = _frame_of(kf, np.random.default_rng(9))
    n = len(kps)
    Rz = np.diag([-1.0, -1.0, 1.0])
    R0, t0 = Rz @ mr.rot("y", 0.3) @ mr.rot("x", -0.2), np.asarray(kf["t"], np.float64) + np.array([0.01, -0.008, 0.012])
    params = M.default_params(480, 640, br.FX, br.FY, br.CX, br.CY)
    mt, mt2 = M.MapTracker(params), M.MapTracker(params)
    d_k, d_d = DeviceBuffer(kps.nbytes).upload(kps), DeviceBuffer(kd.nbytes).upload(kd)
    sizes = []
    everything = dict(min_weight=1, max_neighbours=62, max_fixed=1)
    for frame, cp in ((s.frames[-1], dict(max_neighbours=3)), (s.frames[0], dict(max_neighbours=2)), (s.frames[-1], everything)):
        xyz, desc, ids = cr.local_map(*s.T, frame, (s.S, s.W), **cp)
        sizes.append(len(ids))
        res = s.mb.track_frame_local(mt, frame, d_k, d_d, n, R0, t0, **cp)
        want = mt2.track(xyz, desc, ids, kps, kd, R0, t0)
        _track_equal(res, mt, want, mt2)
        row, lid, _, _ = mt.matches()
        assert (lid[row >= 0] == ids[row[row >= 0]]).all() and (row < len(ids)).all()
        again = s.mb.track_frame_local(mt, frame, d_k, d_d, n, R0, t0, **cp)
        _track_equal(again, mt, want, mt2)
        print(frame, cp, len(ids), {k: res[k] for k in ("status", "n_visible", "n_matches", "n_inliers")})
        if frame == s.frames[-1]:
            assert res["n_matches"] >= 40 and res["status"] in (mr.OK, mr.FEW_INLIERS)          # the refinement ran: every stage is compared
    # the last call's U is the whole table: track_frame's answer
    nlm = len(s.T[1]["id"])
    assert 0 < sizes[0] < nlm and 0 < sizes[1] < nlm and sizes[2] == nlm, sizes
    res = s.mb.track_frame_local(mt, s.frames[-1], d_k, d_d, n, R0, t0, **everything)
    whole = s.mb.track_frame(mt2, d_k, d_d, n, R0, t0)
    _track_equal(res, mt, whole, mt2)
    s.unchanged()
    d_k.free(); d_d.free(); mt.close(); mt2.close()


def test_argument_errors_leave_the_map_untouched(scenes):
    from dvslam_amd import DvsError, BAProblem, map_track as M
    s = scenes("two")
    mt = M.MapTracker(M.default_params(480, 640, br.FX, br.FY, br.CX, br.CY))
    ba = BAProblem.empty()
    frame = s.frames[-1]
    R, t = np.eye(3), np.zeros(3)
    bad = [dict(min_weight=0), dict(max_neighbours=-1), dict(max_neighbours=63), dict(max_fixed=-1), dict(max_fixed=64), dict(max_neighbours=40, max_fixed=24),
           dict(ba_max_iterations=0)]
    calls = [lambda f, p: s.mb.local_window(f, **p), lambda f, p: s.mb.local_bundle_adjust(f, ba, **p), lambda f, p: s.mb.track_frame_local(mt, f, None, None, 0, R, t, **p)]
    for call in calls:
        for p in bad + [None]:
            with pytest.raises(DvsError) as e:
                call(frame if p is not None else 77, p or {})                 # None: an unknown frame id
            assert e.value.code == -6
    for theta in (0, -3):
        with pytest.raises(DvsError) as e:
            s.mb.covisibility(theta)
        assert e.value.code == -6
    with pytest.raises(TypeError):
        s.mb.local_window(frame, min_wieght=3)
    s.mb.local_window(frame, max_neighbours=40, max_fixed=23)                 # 64 cameras: the limit itself is fine
    s.unchanged()
    ba.close(); mt.close()
