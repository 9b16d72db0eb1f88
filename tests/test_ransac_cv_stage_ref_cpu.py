"""The float64 stage references of tests/ransac_cv_stage_ref.py, checked on the CPU before the kernels are held to them
(tests/test_gpu_ransac_cv_stages.py): against ground truth and hand-worked answers, and against the CPU oracle where it states the same
thing.  The differences between the reference and the oracle measured here are the *_MEASURED figures of the GPU tests (asserted here, on
the GPU tests' own inputs, together with the caps those tests put on their inputs); EXPERIMENTS.md, "RANSAC stage tests, OpenCV
procedure", records them."""
import math
import numpy as np
import pytest
import ransac_cv_stage_ref as ref
import ransac_scenes as rs
import test_gpu_ransac_cv_stages as g
from ransac_stage_ref import rodrigues, update_num_iters


# ------------------------------------------------------------------ 7-point
def test_seven_point_against_the_truth():
    sc = rs.two_view(n=40, outlier_frac=0.0, noise=0.0, seed=2)
    K = np.array([[600.0, 0, 320], [0, 600, 240], [0, 0, 1]]); Ki = np.linalg.inv(K)
    tx = np.array([[0, -sc["t"][2], sc["t"][1]], [sc["t"][2], 0, -sc["t"][0]], [-sc["t"][1], sc["t"][0], 0]])
    Ft = ref.unit(Ki.T @ tx @ sc["R"] @ Ki)
    X = sc["X"].astype(np.float64); X2 = X @ sc["R"].T + sc["t"]                      # exact correspondences: float64 projections of the scene's points
    p1 = (X / X[:, 2:]) @ K.T; p2 = (X2 / X2[:, 2:]) @ K.T
    rng = np.random.Generator(np.random.PCG64(1))
    for _ in range(30):
        idx = rng.choice(40, 7, replace=False)
        models, ratio, sep = ref.seven_point(p1[:, :2], p2[:, :2], idx)
        assert len(models) in (1, 3) and 0 < ratio < 1
        assert min(min(np.abs(ref.unit(F) - Ft).max(), np.abs(ref.unit(F) + Ft).max()) for F in models) < 1e-6
        for F in models:
            assert F[2, 2] == 1.0 and abs(np.linalg.det(ref.unit(F))) < 1e-9


def _f7_inputs():
    """every input the GPU tests hold to F7_BOUND: the RANSAC cases (H samples) and the LMedS scenes (300 samples)"""
    cases = {k: (p, g.H) for k, p in g.fm_cases().items()}
    cases.update({f"lmeds{n}": (rs.lmeds_scene(n), g.LMEDS_ITERS) for n in sorted(set(g.L_SIZES) | set(g.RAGGED_L))})
    return cases


@pytest.mark.parametrize("key", list(_f7_inputs()))
def test_f7_measured_and_gate(oracle, key):
    (p1, p2), Hn = _f7_inputs()[key]
    idx, found = oracle.cv_subsets(p1, p2, 7, Hn)
    assert found == Hn
    left_out, worst = 0, 0.0
    for h in range(found):
        models, ratio, sep = ref.seven_point(p1, p2, idx[h])
        if ratio < g.F7_GATE or sep < g.F7_GATE:
            left_out += 1
            continue
        worst = max(worst, ref.match_sets(models, list(oracle.seven_point(p1, p2, idx[h]))))
    print(f"{key}: left out {left_out} / {found}, reference - oracle {worst:.3e}")
    assert left_out <= g.F7_LEFT_OUT * found
    assert worst <= g.F7_MEASURED and g.F7_BOUND < 1e-6


def _oracle_f_stage(oracle, p1, p2, Hn):
    """what the hypothesis stage hands on, from the oracle's 7-point solver: (models [3 Hn][9], valid, found)"""
    idx, found = oracle.cv_subsets(p1, p2, 7, Hn)
    F = np.zeros((3 * Hn, 9)); valid = np.zeros(3 * Hn, np.int32)
    for h in range(found):
        for k, m in enumerate(oracle.seven_point(p1, p2, idx[h])):
            F[3 * h + k] = np.asarray(m).reshape(9); valid[3 * h + k] = 1
    return F, valid, found


@pytest.mark.parametrize("key", list(g.fm_cases()))
def test_fundamental_inputs_meet_the_caps(oracle, key):
    """on the oracle's models (the kernel's to 1e-8): the in-band points of a case and the half-integer margin of its loop"""
    p1, p2 = g.fm_cases()[key]
    F, valid, found = _oracle_f_stage(oracle, p1, p2, g.H)
    thr2 = float(np.float32(g.THR_F ** 2))
    sb = np.array([ref.count_float(ref.epipolar_error(F[m], p1, p2), thr2) if valid[m] else (0, 0) for m in range(3 * g.H)])
    assert sb[:, 1].sum() <= g.BAND_CAP
    best, it, cnt, more, margin = ref.replay_select_cv(sb[:, 0], len(p1), 7, g.CONF, 3, found, 1000)
    print(f"{key}: in band {sb[:, 1].sum()}, select {(best, it, cnt, more)}, margin {margin:.3g}")
    assert best >= 0 and margin > 1e-6


def test_loop_scenes_want_what_the_two_pass_test_needs(oracle):
    F, mask, sel = oracle.find_fundamental_cv(*rs.loop_scene(0.5), g.THR_F, g.CONF, 1000)
    assert 96 < sel[1] < 1000
    F, mask, sel = oracle.find_fundamental_cv(*rs.loop_scene(0.1), g.THR_F, g.CONF, 1000)
    assert sel[1] < 96


# ------------------------------------------------------------------ select and LMedS on hand-made inputs
def test_update_num_iters_hand_values():
    for m, w, q, it in ((7, 0.9, 7.08, 7), (7, 0.8, 19.57, 20), (7, 0.5, 587.2, 587), (5, 0.9, 5.16, 5), (5, 0.8, 11.60, 12)):
        got, quo = update_num_iters(0.99, 1 - w, m, 1000)
        assert got == it and abs(quo - q) < 0.05, (m, w, got, quo)            # (587.2: 587.16)
    assert update_num_iters(0.99, 0.45, 7, 1000)[0] == g.LMEDS_ITERS


@pytest.mark.parametrize("case", ref.SELECT_CV_CASES, ids=[c["name"] for c in ref.SELECT_CV_CASES])
def test_replay_select_cv_on_hand_made_counts(case):
    got = ref.replay_select_cv(case["counts"], ref.SELECT_CV_N, case["model_points"], ref.SELECT_CV_CONFIDENCE, case["group"], case["found"], case["max_iters"])
    assert got[:4] == case["expect"] and got[4] > 1e-6


def test_lmeds_on_hand_made_models():
    """pure x-translation models F(c): the error of a correspondence (x, y) -> (x', y') is (y' - y - c)^2, the same for both lines"""
    def model(c):
        return np.array([0, 0, 0, 0, 0, -1.0, 0, 1.0, c])
    n = 10
    p1 = np.stack([np.arange(n) * 10.0, np.arange(n) * 7.0], 1)
    dy = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.5, 1.0, 2.0, 3.0, 4.0])                # |dy| sorted: index n // 2 = 5 is 0.5
    p2 = p1 + np.stack([np.full(n, 3.0), dy], 1)
    F = np.stack([model(0.0), model(0.25), model(0.25), model(9.0), model(0.1)])
    e0 = ref.epipolar_error(F[0], p1, p2)
    assert np.allclose(e0, dy ** 2, atol=1e-12)
    out = ref.lmeds(F, [1, 1, 1, 1, 0], p1, p2, n)
    # medians: c = 0 -> 0.25 (upper median: sorted index 5; the lower one would be 0); c = 0.25 -> sorted |dy - 0.25| = .25 x 6, .75, ... -> 0.0625;
    # c = 9 -> 81; model 4 (median 0.01) is invalid.  The first of the two equal medians wins.
    assert np.allclose(out["medians"][:4], [0.25, 0.0625, 0.0625, 81.0]) and np.isnan(out["medians"][4])
    assert out["winner"] == 1 and out["gap"] == 0.0
    sigma = 2.5 * 1.4826 * (1 + 5.0 / 3) * 0.25
    assert abs(out["thr2"] - sigma * sigma) < 1e-12
    assert out["count"] == int(((dy - 0.25) ** 2 <= sigma * sigma).sum()) == 8 and out["success"] == 1
    # a model that fits more than half of the points exactly: median 0, sigma at its floor, only those points are inliers — six of them: no success
    dy2 = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 2.0, 3.0, 4.0])
    q2 = p1 + np.stack([np.full(n, 3.0), dy2], 1)
    out = ref.lmeds(F[:1], [1], p1, q2, n)
    assert out["median"] == 0.0 and abs(out["thr2"] - 1e-6) < 1e-18 and out["count"] == 6 and out["success"] == 0 and out["gap"] == math.inf
    assert ref.lmeds(F[:1], [0], p1, q2, n)["winner"] == -1


def test_count_float_band():
    t = 4.0
    e = np.array([0.0, 3.9, 4.0 * (1 - 2e-6), 4.0 * (1 - 0.5e-6), 4.0, 4.0 * (1 + 0.5e-6), 4.0 * (1 + 2e-6), 9.0, np.inf])
    assert ref.count_float(e, t) == (3, 3)


@pytest.mark.parametrize("n", g.L_SIZES + tuple(sorted(set(g.RAGGED_L) - set(g.L_SIZES))))
def test_lmeds_inputs_meet_the_caps(oracle, n):
    p1, p2 = rs.lmeds_scene(n)
    F, valid, found = _oracle_f_stage(oracle, p1, p2, g.LMEDS_ITERS)
    assert found == g.LMEDS_ITERS
    out = ref.lmeds(F, valid, p1, p2, n)
    print(f"n = {n}: winner {out['winner']}, median {out['median']:.3g}, gap {out['gap']:.3g}, count {out['count']}")
    if n == 14:
        assert out["gap"] > 1e-3 and ref.count_float(out["errors"], float(np.float32(out["thr2"])))[1] == 0
    else:
        assert out["median"] < 1e-6


# ------------------------------------------------------------------ PnP
def test_proj_err_float_hand_values():
    K4 = [600.0, 600.0, 320.0, 240.0]
    X = np.array([[0.1, 0, 2.0], [0, 0, -1.0], [1.0, 1.0, 0.0]], np.float32)
    uv = np.array([[353.0, 244.0], [320.0, 240.0], [920.0, 845.0]], np.float32)
    e = ref.proj_err_float(np.eye(3), [0, 0, 0], K4, X, uv)
    # (350, 240) against (353, 244): 25; a point BEHIND the camera on the axis projects onto the principal point: 0 (no depth test);
    # z == 0: 1 / z := 1, the projection is (920, 840)
    assert e.dtype == np.float32 and e.tolist() == [25.0, 0.0, 25.0]


def test_epnp5_recovers_the_true_pose_on_noise_free_samples(oracle):
    """the same bar and the same reason as test_oracle_epnp_and_iterative_refit_on_exact_data (tests/test_ransac.py)"""
    X, uv, K4, behind, R, t = rs.pnp_scene(257, noise=0.0, outliers=0.0)
    idx = oracle.cv_subsets_nocheck(len(X), 5, g.H)
    clean = [h for h in range(g.H) if not set(idx[h].tolist()) & set(behind.tolist())]
    assert len(clean) > 0.7 * g.H
    rt = rodrigues(R)
    for h in clean:
        r, tt, gap45, gap_err, gn_step = ref.epnp5(X[idx[h]], uv[idx[h]], K4)
        assert max(np.abs(r - rt).max(), np.abs(tt - t).max()) <= g.TRUE_POSE_TOL, h
        ro, to = oracle.epnp(X[idx[h]], uv[idx[h]], K4)
        assert max(np.abs(ro - rt).max(), np.abs(to - t).max()) <= g.TRUE_POSE_TOL, h


def _inlier_sets(oracle):
    """the inlier sets the oracle's estimator refits on, per PnP case of the GPU tests"""
    out = {}
    for key, (X, uv, K4, behind, R, t) in g.pnp_cases().items():
        ok, rv, tv, inl, sel, m6 = oracle.solve_pnp_ransac_cv(X, uv, K4, g.H, g.THR_P, g.CONF)
        out[key] = (X[inl].astype(np.float64), uv[inl].astype(np.float64), K4)
    return out


def _planar_sets():
    out = {}
    for n in (65, 257):
        for noise in (0.5, 0.0):
            X, uv, K4, R, t = rs.planar_inlier_set(n, noise)
            out[f"planar_set{n}_{noise}"] = (X.astype(np.float64), uv.astype(np.float64), K4)
    return out


def test_init_measured(oracle):
    """the estimator's inlier sets of the PLANAR cases, which the issue names, are left out and rs.planar_inlier_set stands in for them (see
    INIT_MEASURED): so the initialisation the estimator actually takes on planar65 and planar257 — DLT on a nearly planar set — has no
    bound of its own; only the refit's final pose (REFIT_BOUND) holds it."""
    sets = {k: v for k, v in _inlier_sets(oracle).items() if "planar" not in k}      # (the planar cases' sets: see INIT_MEASURED)
    sets.update(_planar_sets())
    worst = 0.0
    for key, (Xi, uvi, K4) in sets.items():
        path, r0, t0 = ref.refit_init(Xi, uvi, K4)
        ok, r, t, po, ro, to = oracle.solve_pnp_iterative_init(Xi, uvi, K4)
        if len(Xi) < 6:
            assert key in ("n6", "n7") and path == 0 and po == 0 and not ok            # five inliers that are not planar: no initialisation
            continue
        d = max(np.abs(r0 - ro).max(), np.abs(t0 - to).max())
        print(f"{key}: {len(Xi)} points, path {path}, reference - oracle {d:.3e}")
        assert path == po == (1 if key.startswith("planar_set") else 2), key
        worst = max(worst, d)
    assert worst <= g.INIT_MEASURED


def test_refit_init_on_noise_free_data_is_the_true_pose():
    for planar in (False, True):
        if planar:
            X, uv, K4, R, t = rs.planar_inlier_set(257, noise=0.0)
        else:
            X, uv, K4, behind, R, t = rs.pnp_scene(600, noise=0.0, outliers=0.0)
            keep = np.setdiff1d(np.arange(600), behind)[:257]
            X, uv = X[keep], uv[keep]
        path, r0, t0 = ref.refit_init(X, uv, K4)
        assert path == (1 if planar else 2)
        assert max(np.abs(r0 - rodrigues(R)).max(), np.abs(t0 - t).max()) < 1e-5      # float32 inputs, hundreds of points
    X, uv, K4, R, t = rs.planar_inlier_set(12, noise=0.0)
    assert ref.refit_init(X[:3], uv[:3], K4)[0] == 0 and ref.refit_init(X[:4], uv[:4], K4)[0] == 1 and ref.refit_init(X[:5], uv[:5], K4)[0] == 1
    X, uv, K4, behind, R, t = rs.pnp_scene(600, noise=0.0, outliers=0.0)
    keep = np.setdiff1d(np.arange(600), behind)[:6]
    assert ref.refit_init(X[keep[:5]], uv[keep[:5]], K4)[0] == 0 and ref.refit_init(X[keep], uv[keep], K4)[0] == 2


def test_refit_measured(oracle):
    worst = 0.0
    for key, (Xi, uvi, K4) in _inlier_sets(oracle).items():
        if len(Xi) < 6:
            continue
        path, r0, t0 = ref.refit_init(Xi, uvi, K4)
        ro, to = ref.refit_optimum(Xi, uvi, K4, r0, t0)
        ok, r, t = oracle.solve_pnp_iterative(Xi, uvi, K4)
        d = max(np.abs(ro - r).max(), np.abs(to - t).max())
        print(f"{key}: {len(Xi)} inliers, path {path}, oracle - optimum {d:.3e}")
        assert ok
        worst = max(worst, d)
    assert worst <= g.REFIT_MEASURED


@pytest.mark.parametrize("key", [k for k in g.pnp_cases()])
def test_pnp_inputs_meet_the_caps(oracle, key):
    """on the oracle's EPnP models: the in-band points of a case and the half-integer margin of its loop"""
    X, uv, K4, behind, R, t = g.pnp_cases()[key]
    idx = oracle.cv_subsets_nocheck(len(X), 5, g.H)
    thr2 = float(np.float32(g.THR_P ** 2))
    sb = []
    for h in range(g.H):
        r, tt = oracle.epnp(X[idx[h]], uv[idx[h]], K4)
        sb.append(ref.count_float(ref.proj_err_float(ref.rodrigues_to_R(r), tt, K4, X, uv).astype(np.float64), thr2))
    sb = np.array(sb)
    assert sb[:, 1].sum() <= g.BAND_CAP
    best, it, cnt, more, margin = ref.replay_select_cv(sb[:, 0], len(X), 5, g.CONF, 1, g.H, g.H)
    print(f"{key}: in band {sb[:, 1].sum()}, select {(best, it, cnt, more)}, margin {margin:.3g}")
    assert best >= 0 and more == 0 and margin > 1e-6
