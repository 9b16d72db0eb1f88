"""Relocalisation on the GPU against tests/reloc_ref.py.  Stages 1-3 bit for bit through the per-landmark hook and dvs_reloc_get_pairs, at
the sizes where the matrix-core matcher's tiles end (128-row chunks of keypoints, 256 landmark rows per workgroup of the NQ = 2
instantiation a single job launches) and on crafted rows; then the whole rule on one synthetic scene: stage 4 byte for byte against
dvs_solve_pnp_ransac on the gathered list, stage 5 byte for byte against a separate dvs_maptrack_track_device call, the pose against the
truth, and the status paths.  tests/test_reloc_cpu.py asserts, without a GPU, every condition on the scenes that these tests rely on."""
import numpy as np
import pytest
import map_track_ref as mr
import reloc_ref as rr

pytestmark = pytest.mark.gpu
NO_STAGE_4 = 1 << 30           # min_pairs no list reaches: stages 1-3 alone, status FEW_PAIRS


@pytest.fixture(scope="module")
def mt(gpu):
    from dvslam_amd import map_track as M
    h = M.MapTracker(M.default_params(rr.ROWS, rr.COLS, rr.FX, rr.FY, rr.CX, rr.CY), hooks=True)
    yield h
    h.close()


@pytest.fixture(scope="module")
def make(gpu):
    """Relocalizer handles by parameter overrides, kept for the module"""
    from dvslam_amd import reloc as RL
    made = {}

    def get(**kw):
        key = tuple(sorted(kw.items()))
        if key not in made:
            made[key] = RL.Relocalizer(RL.default_params(rr.FX, rr.FY, rr.CX, rr.CY, **kw), hooks=True)
        return made[key]
    yield get
    for h in made.values():
        h.close()


def _check_stages(rl, res, want):
    rec = rl.landmark_records()
    for f in rr.LM_RECORD.names:
        assert rec[f].tobytes() == want["rec"][f].tobytes(), f
    row, kp, dist, inl = rl.pairs()
    assert row.tobytes() == want["lm_row"].tobytes() and kp.tobytes() == want["kp_index"].tobytes() and dist.tobytes() == want["dist"].tobytes()
    assert (res["n_proposed"], res["n_pairs"]) == (want["n_proposed"], want["n_pairs"])
    return inl


def _few_pairs(res):
    assert res["status"] == rr.FEW_PAIRS and res["pnp_inliers"] == 0 and res["pnp_success"] == 0
    assert not res["pnp_R"].any() and not res["pnp_t"].any() and bytes(res["raw"][120:248]) == bytes(128)
    assert np.array_equal(res["R"], np.eye(3)) and not res["t"].any()


@pytest.mark.parametrize("n_kp", [1, 2, 127, 128, 129, 300])
@pytest.mark.parametrize("n_lm", [1, 127, 128, 129, 257])
def test_stages_1_to_3_at_the_tile_edges_with_ties(make, mt, n_lm, n_kp):
    xyz, ld, kps, kd = rr.tie_scene(n_lm, n_kp, 100 * n_lm + n_kp)
    for ratio_pct in (75, 0):
        rl = make(ratio_pct=ratio_pct, min_pairs=NO_STAGE_4)
        res = rl.locate(mt, xyz, ld, None, kps, kd)
        inl = _check_stages(rl, res, rr.stages123(rr.params(ratio_pct=ratio_pct), xyz, ld, kps, kd))
        _few_pairs(res)
        assert not inl.any()


def test_crafted_rows_ids_and_no_ids(make, mt):
    P = rr.params()
    xyz, ld, kps, kd, rows = rr.special_scene(P)
    want = rr.stages123(P, xyz, ld, kps, kd)
    rl = make(min_pairs=NO_STAGE_4)
    res = rl.locate(mt, xyz, ld, None, kps, kd)
    _check_stages(rl, res, want)
    rec = rl.landmark_records()
    assert not rec[rows["ratio_eq"][0]]["proposed"] and rec[rows["ratio_in"][0]]["kept"] and rec[rows["at_max_m1"][0]]["kept"]
    assert not rec[rows["at_max"][0]]["proposed"] and rec[rows["crowd"]]["kept"].sum() == 1 and rec[rows["crowd"][1]]["kept"]
    assert (rec[rows["not_finite"]]["best_k"] == -1).all() and list(rec[rows["dup"]]["kept"]) == [1, 0, 0]
    ids = np.arange(len(xyz), dtype=np.int64) * 5 + 11
    with_ids = rl.locate(mt, xyz, ld, ids, kps, kd)
    _check_stages(rl, with_ids, want)
    assert with_ids["raw"] == res["raw"]
    for ratio_pct in (0, -5):
        off = make(ratio_pct=ratio_pct, min_pairs=NO_STAGE_4)
        _check_stages(off, off.locate(mt, xyz, ld, None, kps, kd), rr.stages123(P.with_(ratio_pct=ratio_pct), xyz, ld, kps, kd))
        assert off.landmark_records()[rows["ratio_eq"][0]]["proposed"]


def test_host_form_refuses_what_map_tracking_refuses(make, mt):
    from dvslam_amd._lib import DvsError
    xyz, ld, kps, kd = rr.tie_scene(20, 10, 1)
    rl = make(min_pairs=NO_STAGE_4)
    out = kps.copy(); out["x"][3] = rr.COLS
    with pytest.raises(DvsError) as e:
        rl.locate(mt, xyz, ld, None, out, kd)
    assert e.value.code == -6
    ids = np.arange(20, dtype=np.int64); ids[7] = ids[6]
    with pytest.raises(DvsError) as e:
        rl.locate(mt, xyz, ld, ids, kps, kd)
    assert e.value.code == -6
    assert rl.locate(mt, xyz[:0], ld[:0], None, kps, kd)["n_pairs"] == 0 and rl.locate(mt, xyz, ld, None, kps[:0], kd[:0])["n_pairs"] == 0      # empty sides
    assert len(rl.landmark_records()) == 20 and (rl.landmark_records()["best_k"] == -1).all()


# ---------------------------------------------------------------------------------------------------- end to end
class _Dev:
    def __init__(self, s):
        from dvslam_amd._lib import DeviceBuffer
        self.bufs = [DeviceBuffer(np.ascontiguousarray(s[k]).nbytes).upload(np.ascontiguousarray(s[k])) for k in ("xyz", "ldesc", "ids", "kps", "kdesc")]
        self.n_lm, self.n_kp = len(s["xyz"]), len(s["kps"])

    def args(self, ids=True):
        b = self.bufs
        return (b[0], b[1], b[2] if ids else None, self.n_lm, b[3], b[4], self.n_kp)

    def free(self):
        for b in self.bufs:
            b.free()


@pytest.fixture(scope="module")
def scene():
    return rr.scene()


@pytest.fixture(scope="module")
def e2e(make, mt, scene):
    """one locate call on the scene and everything read back after it; the product's own RANSAC on the gathered list"""
    from dvslam_amd import FrontendGlue
    s = scene
    dev = _Dev(s)
    rl = make()
    res = rl.locate_device(mt, *dev.args())
    row, kp, dist, inl = rl.pairs()
    out = dict(res=res, rec=rl.landmark_records(), row=row, kp=kp, dist=dist, inl=inl, pnp=rl.pnp_record(), matches=mt.matches(), dev=dev, rl=rl)
    want = rr.stages123(s["P"], s["xyz"], s["ldesc"], s["kps"], s["kdesc"])
    g = FrontendGlue()
    P = s["P"]
    out["want"] = want
    out["solo"] = g.solve_pnp_ransac(want["obj"], want["img"], P.K4, P.pnp_iterations, P.pnp_reproj_err, P.pnp_confidence, seed=P.seed)
    yield out
    dev.free()


def test_scene_stages_1_to_3(e2e):
    _check_stages(e2e["rl"], e2e["res"], e2e["want"])


def test_scene_stage_4_is_the_products_ransac_on_the_list(e2e, scene):
    ok, rvec, tvec, inl = e2e["solo"]
    assert ok, "dvs_solve_pnp_ransac must succeed on the scene's list at the default iterations"
    res = e2e["res"]
    ok2, rvec2, tvec2, n2 = e2e["pnp"]
    assert ok2 and res["pnp_success"] == 1 and res["pnp_inliers"] == n2 == len(inl)
    assert rvec2.tobytes() == rvec.tobytes() and tvec2.tobytes() == tvec.tobytes()
    flags = np.zeros(len(e2e["inl"]), np.uint8); flags[inl] = 1
    assert e2e["inl"].tobytes() == flags.tobytes()
    assert not e2e["inl"][rr.wrong_pairs(scene, e2e["want"])].any() and res["pnp_inliers"] >= 100
    R, t = rr.rodrigues_pose(rvec2, tvec2)
    dR, dt = float(np.abs(res["pnp_R"] - R).max()), float(np.abs(res["pnp_t"] - t).max())
    print(f"host conversion against the restatement: R {dR:.2e} t {dt:.2e}")
    assert dR <= 10 * rr.POSE_MEASURED and dt <= 10 * rr.POSE_MEASURED
    assert dR <= 1e-12 and dt <= 1e-12          # two FP64 evaluations of one formula: sin and cos within an ulp of each other, |t| of a few metres


def test_scene_stage_5_is_a_separate_track_call(e2e, scene, gpu):
    from dvslam_amd import map_track as M
    s, res = scene, e2e["res"]
    assert res["status"] == rr.OK
    other = M.MapTracker(M.default_params(rr.ROWS, rr.COLS, rr.FX, rr.FY, rr.CX, rr.CY), hooks=True)
    sep = other.track_device(*e2e["dev"].args(), res["pnp_R"], res["pnp_t"])
    tr = res["track"]
    assert all(np.asarray(tr[k]).tobytes() == np.asarray(sep[k]).tobytes() for k in sep)
    assert res["R"].tobytes() == sep["R"].tobytes() and res["t"].tobytes() == sep["t"].tobytes()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(e2e["matches"], other.matches()))
    other.close()
    assert tr["status"] == mr.OK and tr["n_inliers"] >= s["P"].min_confirmed
    row, _, _, inl = e2e["matches"]
    ks = np.flatnonzero(row >= 0)
    X = np.array([[float(v) for v in s["xyz"][j]] for j in row[ks]]); px = np.array([[float(s["kps"][k]["x"]), float(s["kps"][k]["y"])] for k in ks])
    Rcw, tcw = mr.pose_cw(tr["R"], tr["t"])
    opt = mr.scipy_optimum(s["MP"], Rcw, tcw, X, px, s["kps"]["octave"][ks], inl[ks])
    assert abs(tr["cost"] - opt) <= 1e-6 * opt, (tr["cost"], opt)


def test_scene_pose_against_the_truth(e2e, scene):
    res = e2e["res"]
    err = max(float(np.abs(res["R"] - scene["R_true"]).max()), float(np.abs(res["t"] - scene["t_true"]).max()))
    print(f"pose error {err:.3e} (bound {10 * rr.POSE_MEASURED:.1e})")
    assert err <= 10 * rr.POSE_MEASURED


def test_two_identical_calls_give_identical_bytes(e2e, mt):
    again = e2e["rl"].locate_device(mt, *e2e["dev"].args())
    assert again["raw"] == e2e["res"]["raw"] and len(again["raw"]) == 344
    no_ids = e2e["rl"].locate_device(mt, *e2e["dev"].args(ids=False))
    assert no_ids["raw"] == e2e["res"]["raw"]                  # the ids name the landmarks in the tracker's matches, nothing else
    row, kp, dist, inl = e2e["rl"].pairs()
    assert row.tobytes() == e2e["row"].tobytes() and inl.tobytes() == e2e["inl"].tobytes()


# ---------------------------------------------------------------------------------------------------- status paths
def _locate(rl, mt, s):
    return rl.locate(mt, s["xyz"], s["ldesc"], s["ids"], s["kps"], s["kdesc"])


def test_a_random_frame_finds_no_pairs(make, mt, scene):
    s = rr.random_frame(scene)
    res = _locate(make(), mt, s)
    want = rr.stages123(s["P"], s["xyz"], s["ldesc"], s["kps"], s["kdesc"])
    assert want["n_pairs"] < s["P"].min_pairs and res["n_pairs"] == want["n_pairs"]
    _few_pairs(res)


def test_one_pair_short_of_min_pairs(make, mt, scene):
    P = scene["P"]
    s = rr.cut_to_pairs(scene, P.min_pairs - 1)
    rl = make()
    res = _locate(rl, mt, s)
    assert res["n_pairs"] == P.min_pairs - 1
    _few_pairs(res)
    ok, rvec, tvec, n = rl.pnp_record()
    assert not ok and n == 0 and not rvec.any() and not tvec.any()                      # nothing was solved
    assert _locate(rl, mt, rr.cut_to_pairs(scene, P.min_pairs))["status"] != rr.FEW_PAIRS


def test_pairs_that_are_all_wrong_give_no_pose(make, mt, scene):
    s = rr.all_wrong(scene)
    rl = make()
    res = _locate(rl, mt, s)
    want = rr.stages123(s["P"], s["xyz"], s["ldesc"], s["kps"], s["kdesc"])
    _check_stages(rl, res, want)
    assert rr.wrong_pairs(s, want).all()
    assert res["status"] == rr.NO_POSE and (res["pnp_success"] == 0 or res["pnp_inliers"] < s["P"].min_pnp_inliers)
    assert not res["pnp_R"].any() and not res["pnp_t"].any() and bytes(res["raw"][120:248]) == bytes(128)
    assert np.array_equal(res["R"], np.eye(3)) and not res["t"].any()


def test_a_confirmation_that_asks_for_more_inliers_than_there_are(make, mt, scene, e2e):
    n = e2e["res"]["track"]["n_inliers"]
    res = make(min_confirmed=n + 1).locate_device(mt, *e2e["dev"].args())
    assert res["status"] == rr.NOT_CONFIRMED and np.array_equal(res["R"], np.eye(3)) and not res["t"].any()
    assert res["raw"][4:248] == e2e["res"]["raw"][4:248]                                                      # everything but the status and R, t
    assert res["track"]["status"] == mr.OK and res["track"]["n_inliers"] == n
    assert res["pnp_R"].tobytes() == e2e["res"]["pnp_R"].tobytes()                                             # track's prior: the PnP pose's bytes
    assert make(min_confirmed=n).locate_device(mt, *e2e["dev"].args())["status"] == rr.OK
