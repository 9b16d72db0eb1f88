"""Loop verification on the GPU (csrc/loop_verify.hip) STAGE BY STAGE against the sequential float64 statement tests/loop_verify_ref.py.
Every stage is fed with the GPU's own output of the stage before it (dvs_test_loop_verify_stages, include/dvslam_hip_test_loop.h: the
product's launch sequence plus what each stage left on the device):

  gather      list rows and the six coordinate planes: exact.  The query and every entry carry points without depth (NaN, z = 0, z < 0,
              +-inf), partners past the entry's last row, and, behind the query's count, rows that WOULD be perfect inliers.
  hypotheses  sample positions: exact.  The degenerate flag: equal (no gap of the scenes lies in vr.GAP_FLAG_BAND, asserted on the CPU).
              (R, t): within 10 x vr.HORN_MEASURED / gap for the gated hypotheses (gap >= vr.GAP_GATE) — HORN_MEASURED is the distance
              between two float64 statements, neither of them the kernel, measured by tests/test_loop_verify_cpu.py; an eigenvector's
              error scales with 1 / gap; ten times is the margin tests/test_gpu_ransac_stages.py gives, for the same reason.
  score       counts of the GPU's own models: equal (no error of theirs may lie within reproj_err^2 (1 +- 1e-9): asserted per model).
  select      vr.replay_select over the GPU's counts: equal, the iteration counts' rounding margin asserted.
  refine      every round from the GPU's model in hand: set size, acceptance and flag equal, the model within 10 x vr.REFINE_MEASURED /
              gap; the `refused` case ends in a round that loses inliers and is turned down.
  result      count, mask, success, iterations: equal; tvec: the model in hand's bytes; rvec against vr.rodrigues (1e-12: the conversion
              is ransac_shared.h's, held to its own reference elsewhere); rms_px to 1e-9 relative.

The planted pose is recovered within vr.POSE_TOL_RAD / vr.POSE_TOL_M, derived in loop_verify_ref.py from the scene's noise alone (0.5 px
and 0.2 % of the depth on the query side: 5 standard deviations of the least-squares estimate over the 179 inliers of the smallest case)."""
import ctypes as C
import functools
import math
import numpy as np
import pytest

import loop_ref as lr
import loop_verify_ref as vr

pytestmark = pytest.mark.gpu
THR2 = 16.0


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _params(d):
    from dvslam_amd import LoopVerifyParams
    return LoopVerifyParams(**d)


@functools.lru_cache(maxsize=None)
def _world():
    """the scene, and one database through the test library that holds every entry of vr.ENTRIES (random descriptor rows: the matches come
    from the scene, not from the descriptors) with its points — except `nopoints`, which never gets any"""
    from dvslam_amd import OrbVocabulary, LoopDatabase, bow
    from dvslam_amd._lib import test_lib
    voc, _, _ = lr.standard_scene()
    product = bow.lib
    bow.lib = test_lib            # the vocabulary, and the database over it, make ALL their calls through the test library: the stage
    try:                          # hook takes a handle of the library that exports it
        g = OrbVocabulary.from_arrays(voc.k, voc.L, voc.parent, voc.is_leaf, voc.desc, voc.weight, voc.scoring, voc.weighting)
    finally:
        bow.lib = product
    db = LoopDatabase(g, 1)
    query, entries, rq = vr.make_scene()
    rng = np.random.default_rng(77)
    for k, (name, _, _) in enumerate(vr.ENTRIES):
        e = entries[name]
        assert db.add(rng.integers(0, 256, (e["rows"], 32), dtype=np.uint8)) == k
        if name != "nopoints":
            db.set_points(k, e["e_xyz"])
    return test_lib(), g, db, query, entries, rq


def run_stages(q, names, P, cap):
    """dvs_test_loop_verify_stages for the candidates `names` (None: an id out of range) in `cap` slots"""
    L, g, db, _, entries, _ = _world()
    S, H = q["stride"], P["iterations"]
    ids = np.array([vr.ENTRY_ID[x] if x is not None else len(vr.ENTRIES) + 5 for x in names], np.int32)
    train = np.full((cap, S), -1, np.int32)
    for c, x in enumerate(names):
        if x is not None:
            train[c] = entries[x]["train"]
    train[len(names):] = entries["m600"]["train"]     # the slots past the count hold a perfectly good match: they must not be looked at
    from dvslam_amd._lib import LOOP_VERIFY_RESULT
    o = dict(res=np.zeros(cap, LOOP_VERIFY_RESULT), mask=np.zeros((cap, S), np.uint8), n_list=np.full(cap, -7, np.int32),
             list_i=np.full((cap, S), -7, np.int32), pts=np.zeros((cap, 6, S), np.float32), sample=np.full((cap, H, 3), -7, np.int32),
             valid=np.full((cap, H), -7, np.int32), models=np.full((cap, H, 12), np.nan), gap=np.zeros((cap, H)),
             counts=np.full((cap, H), -7, np.int32), sel=np.full((cap, 4), -7, np.int32), rounds=np.full((cap, 9, 16), np.nan))
    pp = _params(P)
    rc = L.dvs_test_loop_verify_stages(db._h, _p(q["q_xyz"]), q["n"], S, _p(ids), len(names), cap, _p(train), C.byref(pp), _p(o["res"]), _p(o["mask"]),
                                       _p(o["n_list"]), _p(o["list_i"]), _p(o["pts"]), _p(o["sample"]), _p(o["valid"]), _p(o["models"]), _p(o["gap"]),
                                       _p(o["counts"]), _p(o["sel"]), _p(o["rounds"]))
    assert rc == 0, L.dvs_last_error()
    return o


def _failed(res, mask, n_corr):
    assert (int(res["n_corr"]), int(res["n_inliers"]), int(res["success"]), int(res["iterations"])) == (n_corr, 0, 0, 0)
    assert not res["rvec"].any() and not res["tvec"].any() and res["rms_px"] == 0.0 and not mask.any()


def check_candidate(o, c, q, name, P, figures):
    """slot c of a stage run against the reference, each stage on the GPU's own previous stage"""
    _, _, _, _, entries, _ = _world()
    e = entries[name]
    res, mask = o["res"][c], o["mask"][c]
    e_xyz = e["e_xyz"] if name != "nopoints" else np.full_like(e["e_xyz"], np.nan)
    li, lj = vr.gather(q["q_xyz"], q["n"], e["train"], e_xyz)
    m = len(li)
    # ---- gather
    assert o["list_i"][c, :m].tolist() == li.tolist()
    if m:
        want = np.concatenate([e_xyz[lj].T, q["q_xyz"][li].T])
        assert o["pts"][c, :, :m].tobytes() == np.ascontiguousarray(want).tobytes()
    if m < P["min_correspondences"]:
        assert o["n_list"][c] == 0 and (o["valid"][c] == 0).all() and (o["counts"][c] == 0).all() and o["sel"][c, 0] == -1
        assert not o["rounds"][c].any()
        _failed(res, mask, m)
        return
    assert o["n_list"][c] == m and res["n_corr"] == m
    E = o["pts"][c, :3, :m].T.astype(np.float64); Q = o["pts"][c, 3:, :m].T.astype(np.float64)
    # ---- hypotheses and score
    seed_c = vr.candidate_seed(P["seed"], vr.ENTRY_ID[name])
    H = P["iterations"]
    gated = 0
    for h in range(H):
        idx, R, t, gap, ok = vr.hypothesis(E, Q, seed_c, h)
        assert o["sample"][c, h].tolist() == idx
        assert not vr.GAP_FLAG_BAND[0] <= gap <= vr.GAP_FLAG_BAND[1]
        assert bool(o["valid"][c, h]) == ok, (h, gap, o["gap"][c, h])
        M = o["models"][c, h]
        if not ok:
            assert not M.any() and o["counts"][c, h] == 0
            continue
        err = vr.errors(M[:9].reshape(3, 3), M[9:], P["K4"], E, Q)             # the GPU's own model
        if gap >= vr.GAP_GATE:
            gated += 1
            d = max(np.abs(M[:9].reshape(3, 3) - R).max(), np.abs(M[9:] - t).max())
            figures["horn"] = max(figures["horn"], d * gap)
            assert abs(o["gap"][c, h] - gap) <= 1e-9 * max(gap, 1.0)
            assert not vr.in_band(err, THR2)
        elif vr.in_band(err, THR2):
            continue
        assert o["counts"][c, h] == int((err <= THR2).sum()), h
    print(f"{name}: hypotheses |delta (R, t)| x gap = {figures['horn']:.3e} (bound {10 * vr.HORN_MEASURED:.1e})")
    assert figures["horn"] <= 10 * vr.HORN_MEASURED      # d <= 10 HORN_MEASURED / gap for every gated hypothesis
    assert gated >= 0.4 * H                                                      # `dup` flags a third of its samples
    # ---- select
    best, it, bc, margin = vr.replay_select(o["counts"][c], m, 3, P["confidence"], 1)
    assert margin > 1e-6
    assert o["sel"][c].tolist() == [best, it, bc, 0]
    rounds = o["rounds"][c]
    if best < 0:
        assert not rounds.any()
        _failed(res, mask, m)
        return
    # ---- refine
    assert rounds[0, :12].tobytes() == o["models"][c, best].tobytes() and rounds[0, 12:].tolist() == [bc, 1.0, 1.0, 0.0]
    R, t, size = rounds[0, :9].reshape(3, 3), rounds[0, 9:12], bc
    r = 0
    for r in range(1, P["refine_rounds"] + 1):
        Rn, tn, gap, ok, nsize, acc, e_old, e_new = vr.refine_round(R, t, P["K4"], THR2, E, Q)
        assert not vr.in_band(e_old, THR2) and not vr.in_band(e_new, THR2) and gap >= vr.GAP_GATE
        G = rounds[r]
        d = max(np.abs(G[:9].reshape(3, 3) - Rn).max(), np.abs(G[9:12] - tn).max())
        figures["refine"] = max(figures["refine"], d * gap)
        print(f"{name}: round {r} |delta (R, t)| x gap = {d * gap:.3e} (bound {10 * vr.REFINE_MEASURED:.1e})")
        assert d <= 10 * vr.REFINE_MEASURED / gap, (r, d, gap)
        e_gpu = vr.errors(G[:9].reshape(3, 3), G[9:12], P["K4"], E, Q)
        assert not vr.in_band(e_gpu, THR2)
        assert G[12:].tolist() == [int((e_gpu <= THR2).sum()), float(acc), float(ok), 0.0] and G[12] == nsize
        figures["refused"] += 0 if acc else 1
        if not acc:
            break
        R, t, size = G[:9].reshape(3, 3), G[9:12], nsize
    assert not rounds[r + 1:].any()                                              # rounds that did not run
    # ---- result
    err = vr.errors(R, t, P["K4"], E, Q)
    S = err <= THR2
    want_mask = np.zeros(q["stride"], np.uint8); want_mask[li[S]] = 1
    assert mask.tolist() == want_mask.tolist() and not mask[q["n"]:].any()
    assert (int(res["n_inliers"]), int(res["success"]), int(res["iterations"])) == (size, int(size >= P["min_inliers"]), it) and size == S.sum()
    assert res["tvec"].tobytes() == np.ascontiguousarray(t).tobytes()
    assert np.abs(res["rvec"] - vr.rodrigues(R)).max() <= 1e-12
    assert abs(res["rms_px"] - math.sqrt(err[S].mean())) <= 1e-9 * res["rms_px"]
    return R, t


@pytest.mark.parametrize("name,over", vr.CASES, ids=[c[0] for c in vr.CASES])
def test_stages_of_one_candidate(gpu, name, over):
    _, _, _, query, entries, rq = _world()
    q = rq if name == "refused" else query
    P = vr.case_params(over)
    figures = dict(horn=0.0, refine=0.0, refused=0)
    o = run_stages(q, [name], P, 1)
    pose = check_candidate(o, 0, q, name, P, figures)
    print(f"{name}: |delta| x gap hypotheses {figures['horn']:.3e} (bound {10 * vr.HORN_MEASURED:.1e}), refinement {figures['refine']:.3e} "
          f"(bound {10 * vr.REFINE_MEASURED:.1e})")
    assert (figures["refused"] == 1) == (name == "refused")
    if name in ("m255", "m256", "m257", "m600"):
        R, t = pose
        angle = math.acos(min(1.0, (np.trace(R @ vr.POSE_R.T) - 1) / 2))
        assert o["res"][0]["success"] == 1 and angle <= vr.POSE_TOL_RAD and np.linalg.norm(t - vr.POSE_T) <= vr.POSE_TOL_M
        assert abs(int(o["res"][0]["n_inliers"]) - len(entries[name]["inlier_rows"])) <= 0.02 * len(entries[name]["inlier_rows"])


def test_ragged_batch(gpu):
    _, _, _, query, entries, _ = _world()
    P = vr.case_params(dict(iterations=vr.H_CASE))
    cap = len(vr.RAGGED) + 2
    o = run_stages(query, vr.RAGGED, P, cap)
    figures = dict(horn=0.0, refine=0.0, refused=0)
    for c, name in enumerate(vr.RAGGED):
        if name is None:                                                         # an id out of range
            _failed(o["res"][c], o["mask"][c], -1)
            assert o["n_list"][c] == 0 and o["sel"][c, 0] == -1
        else:
            check_candidate(o, c, query, name, P, figures)
    assert [int(x) for x in o["res"]["n_corr"]] == [257, 2, 0, 600, -1, 0, 257, 0, 0]
    assert o["res"]["success"].tolist() == [1, 0, 0, 1, 0, 0, 1, 0, 0]
    for c in range(len(vr.RAGGED), cap):                                         # slots past the count: written, failed
        _failed(o["res"][c], o["mask"][c], 0)
        assert o["n_list"][c] == 0 and o["sel"][c, 0] == -1 and not o["rounds"][c].any()
    assert o["res"][0].tobytes() == o["res"][6].tobytes() and o["mask"][0].tobytes() == o["mask"][6].tobytes()   # the same entry twice
    # ... and the same record as the candidate alone (the seed follows the entry, not the position)
    alone = run_stages(query, ["m257"], P, 1)
    assert alone["res"][0].tobytes() == o["res"][0].tobytes() and alone["mask"][0].tobytes() == o["mask"][0].tobytes()


def test_parameters_on_both_sides_of_the_counts(gpu):
    _, _, _, query, entries, _ = _world()
    base = dict(iterations=vr.H_CASE)
    figures = dict(horn=0.0, refine=0.0, refused=0)
    o0 = run_stages(query, ["m257"], vr.case_params(dict(base, refine_rounds=0)), 1)
    check_candidate(o0, 0, query, "m257", vr.case_params(dict(base, refine_rounds=0)), figures)
    assert not o0["rounds"][0, 1:].any() and o0["res"][0]["n_inliers"] == o0["sel"][0, 2]
    for mc, passes in ((257, True), (258, False)):
        P = vr.case_params(dict(base, min_correspondences=mc))
        o = run_stages(query, ["m257"], P, 1)
        check_candidate(o, 0, query, "m257", P, figures)
        assert (o["res"][0]["success"] == 1) == passes and o["res"][0]["n_corr"] == 257
    nin = int(o0["res"][0]["n_inliers"])
    for mi, ok in ((nin, 1), (nin + 1, 0)):
        P = vr.case_params(dict(base, refine_rounds=0, min_inliers=mi))
        o = run_stages(query, ["m257"], P, 1)
        assert o["res"][0]["success"] == ok and o["res"][0]["n_inliers"] == nin and o["mask"][0].sum() == nin and o["res"][0]["rvec"].any()


def test_host_form_errors_and_identical_bytes(gpu):
    from dvslam_amd._lib import DvsError
    _, _, db, query, entries, _ = _world()
    n = query["n"]
    P = _params(vr.case_params(dict(iterations=vr.H_CASE)))
    ids = [vr.ENTRY_ID["m600"], vr.ENTRY_ID["m255"]]
    train = np.stack([entries["m600"]["train"][:n], entries["m255"]["train"][:n]])
    a = db.verify(query["q_xyz"][:n], ids, train, P)
    b = db.verify(query["q_xyz"][:n], ids, train, P)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()          # two identical calls: identical bytes
    o = run_stages(query, ["m600", "m255"], vr.case_params(dict(iterations=vr.H_CASE)), 2)
    assert a[0].tobytes() == o["res"].tobytes() and a[1].tobytes() == o["mask"][:, :n].tobytes()   # the stride does not change the answer
    assert a[0]["success"].tolist() == [1, 1]
    for bad in (dict(iterations=0), dict(iterations=4097), dict(min_correspondences=2), dict(min_inliers=2), dict(refine_rounds=9),
                dict(reproj_err=0.0), dict(confidence=1.0), dict(K4=(0.0, 615.0, 320.0, 240.0)), dict(reproj_err=math.nan)):
        with pytest.raises(DvsError) as ei:
            db.verify(query["q_xyz"][:n], ids, train, _params(vr.case_params(bad)))
        assert ei.value.code == -6
    with pytest.raises(DvsError) as ei:
        db.verify(query["q_xyz"][:n], [0, len(vr.ENTRIES)], train, P)            # an id out of range: before any device work
    assert ei.value.code == -6
    assert db._L.dvs_loopv_db_verify(db._h, _p(query["q_xyz"]), n, _p(np.array(ids, np.int32)), 2, _p(train), None, _p(a[0]), _p(a[1])) == -6
    with pytest.raises(DvsError) as ei:
        db.set_points(0, entries["m600"]["e_xyz"][:-1])                          # not the entry's row count
    assert ei.value.code == -6
    with pytest.raises(DvsError):
        db.set_points(len(vr.ENTRIES), entries["m600"]["e_xyz"])
    assert db.get_points(0).tobytes() == entries["m600"]["e_xyz"].tobytes()
    assert np.isnan(db.get_points(vr.ENTRY_ID["nopoints"])).all() and len(db.get_points(vr.ENTRY_ID["nopoints"])) == entries["nopoints"]["rows"]


def test_detect_verify_is_detect_then_verify(gpu):
    from dvslam_amd import OrbVocabulary, LoopDatabase
    from dvslam_amd._lib import DeviceBuffer, LOOP_VERIFY_RESULT
    voc, entries, query = lr.standard_scene()
    ref = lr.LoopDatabase(voc, 1)
    for e in entries:
        ref.add(e)
    want = ref.match(query, [0, 1, 2, 3])
    pts, qp = vr.standard_points(entries, query, want[0][1])
    g = OrbVocabulary.from_arrays(voc.k, voc.L, voc.parent, voc.is_leaf, voc.desc, voc.weight, voc.scoring, voc.weighting)
    db, plain = LoopDatabase(g, 1), LoopDatabase(g, 1)
    for k, e in enumerate(entries):
        assert db.add(e) == k and plain.add(e) == k
        db.set_points(k, pts[k])
    # add and detect: the same bytes with and without points stored
    d0, d1 = plain.detect(query, 3), db.detect(query, 3)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(d0, d1))
    assert all(plain.get_descriptors(k).tobytes() == db.get_descriptors(k).tobytes() for k in range(4))
    assert plain.retrieve_features(2) == db.retrieve_features(2)
    P = _params(vr.default_params(iterations=64, seed=3))
    ids, scores, nm, train, dist, res, mask = db.detect_verify(query, qp, P, 3)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(d1, (ids, scores, nm, train, dist)))
    first = ids.tolist().index(1)
    assert res[first]["success"] == 1 and res[first]["n_corr"] == (want[0][1] >= 0).sum() - (want[0][1][3] >= 0) and mask[first].sum() == res[first]["n_inliers"]
    assert np.abs(res[first]["tvec"] - vr.POSE_T).max() < 1e-5                     # noise-free points: float32 rounding only
    assert [int(s) for k, s in enumerate(res["success"]) if k != first] == [0, 0]
    # the host form on the read-back
    r2, m2 = db.verify(qp, ids, train, P)
    assert r2.tobytes() == res.tobytes() and m2.tobytes() == mask.tobytes()
    # the device forms: detect_device, then verify_device on exactly its buffers
    n, S, cap = len(query), len(query) + 19, 4
    rows = np.zeros((S, 32), np.uint8); rows[:n] = query; rows[n:] = entries[1][:S - n]
    xq = np.zeros((S, 3), np.float32); xq[:n] = qp; xq[n:] = pts[1][:S - n]
    d_q, d_x, d_n = DeviceBuffer(rows.nbytes).upload(rows), DeviceBuffer(xq.nbytes).upload(xq), DeviceBuffer(4).upload(np.array([n], np.int32))
    d_ids, d_sc, d_nm, d_nr = DeviceBuffer(cap * 4), DeviceBuffer(cap * 8), DeviceBuffer(cap * 4), DeviceBuffer(4)
    d_tr, d_di = DeviceBuffer(cap * S * 4), DeviceBuffer(cap * S * 4)
    d_res = DeviceBuffer(cap * 72).upload(np.full(cap * 72, 0x5a, np.uint8)); d_mask = DeviceBuffer(cap * S).upload(np.full(cap * S, 0x5a, np.uint8))
    db.detect_device(d_q.ptr, d_n.ptr, S, 3, -1, d_ids.ptr, d_sc.ptr, d_nm.ptr, d_tr.ptr, d_di.ptr, cap, d_nr.ptr)
    db.verify_device(d_x.ptr, d_n.ptr, S, d_ids.ptr, d_nr.ptr, cap, d_tr.ptr, P, d_res.ptr, d_mask.ptr)
    g.synchronize()
    r3 = d_res.download(np.uint8, cap * 72).view(LOOP_VERIFY_RESULT); m3 = d_mask.download(np.uint8, cap * S).reshape(cap, S)
    assert r3[:3].tobytes() == res.tobytes() and m3[:3, :n].tobytes() == mask.tobytes() and not m3[:, n:].any() and not m3[3].any()
    assert r3[3].tobytes() == np.zeros(1, LOOP_VERIFY_RESULT).tobytes()
    db.close(); plain.close(); g.close()


def test_points_round_trip_across_growth_and_clear(gpu):
    from dvslam_amd import OrbVocabulary, LoopDatabase
    from dvslam_amd._lib import DeviceBuffer
    voc, entries, _ = lr.standard_scene()
    g = OrbVocabulary.from_arrays(voc.k, voc.L, voc.parent, voc.is_leaf, voc.desc, voc.weight, voc.scoring, voc.weighting)
    db = LoopDatabase(g, 1)
    rng = np.random.default_rng(9)
    stride = max(len(e) for e in entries[:2]) + 5
    rows = np.zeros((2, stride, 32), np.uint8); xyz = rng.normal(size=(2, stride, 3)).astype(np.float32)
    counts = np.array([len(entries[0]), len(entries[1])], np.int32)
    for f in range(2):
        rows[f, :counts[f]] = entries[f]
    d_rows, d_xyz, d_n = DeviceBuffer(rows.nbytes).upload(rows), DeviceBuffer(xyz.nbytes).upload(xyz), DeviceBuffer(8).upload(counts)
    assert db.add_device(d_rows.ptr, d_n.ptr, stride, 2) == 0
    assert np.isnan(db.get_points(0)).all() and np.isnan(db.get_points(1)).all()     # never given points
    db.set_points_device(0, d_xyz.ptr, d_n.ptr, stride, 2)
    g.synchronize()
    want = [xyz[f, :counts[f]].copy() for f in range(2)]
    assert all(db.get_points(f).tobytes() == want[f].tobytes() for f in range(2))
    short = DeviceBuffer(8).upload(np.array([7, 10 ** 6], np.int32))                  # fewer rows than the entry has; more than the stride
    xyz2 = (xyz + 1).astype(np.float32)
    d_xyz2 = DeviceBuffer(xyz2.nbytes).upload(xyz2)
    db.set_points_device(0, d_xyz2.ptr, short.ptr, stride, 2)
    g.synchronize()
    want[0][:7] = xyz2[0, :7]; want[1] = xyz2[1, :counts[1]]
    assert all(db.get_points(f).tobytes() == want[f].tobytes() for f in range(2))
    for k in range(12):                                                              # the per-row blocks grow several times
        assert db.add(entries[k % 4]) == 2 + k
    assert all(db.get_points(f).tobytes() == want[f].tobytes() for f in range(2))
    assert all(np.isnan(db.get_points(2 + k)).all() and len(db.get_points(2 + k)) == len(entries[k % 4]) for k in range(12))
    db.set_points(13, np.ones((len(entries[3]), 3), np.float32))
    assert (db.get_points(13) == 1).all() and np.isnan(db.get_points(12)).all()
    db.clear()                                                                       # forgets the points too
    assert db.add(entries[0]) == 0 and np.isnan(db.get_points(0)).all()
    db.close(); g.close()
