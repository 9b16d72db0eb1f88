"""The library's own robust estimators (csrc/ransac.hip: dvs_find_fundamental_ransac*, dvs_solve_pnp_ransac*) STAGE BY STAGE, hypothesis by
hypothesis, against the float64 statements of tests/ransac_stage_ref.py.  tests/test_ransac.py holds the estimators to statistical bars
(inlier-set IoU, recall, a pose within milliradians), which RANSAC passes with a broken stage: that is what it is for.  Here every stage
gets the GPU's own output of the stage before it (dvs_test_fm_stages / dvs_test_pnp_stages, include/dvslam_hip_test.h) and is compared
exactly, or to a bound with a stated provenance:

  F_BOUND       hypotheses against ref.eight_point.  Measured on the CPU (EXPERIMENTS.md, "RANSAC stage tests"): the largest max-norm
                difference between ref.eight_point (SVD) and the CPU oracle's eight_point (Jacobi eigenvectors), two float64 statements
                neither of which is the kernel, over the gated hypotheses of every case below = 2.3e-9; the kernel, which eliminates
                with complete pivoting instead, gets ten times that.
  REFINE_BOUND  refined pose against scipy.optimize.least_squares from the same start on the same inliers.  Measured: the CPU oracle's
                refinement against scipy on the scenes below = 3.0e-8 (rvec and tvec entries); the kernel gets ten times that.
  BAND          counts and masks: an error within thr^2 (1 +- 1e-9) may fall either way.  A few dozen float64 operations on coordinates
                of order 1e3 px around a 2 to 4 px threshold give a relative error of about 1e-13; 1e-9 leaves four orders, and the tests
                assert that no point of their inputs lies inside the band, which makes the check an equality.
"""
import ctypes as C
import math
import numpy as np
import pytest
import ransac_scenes as rs
import ransac_stage_ref as ref
from ransac_scenes import fm_scene, pnp_scene

pytestmark = pytest.mark.gpu

H = 200
THR_F, THR_P, CONF = 2.0, 4.0, 0.99
BAND = 1e-9
F_GATE, F_LEFT_OUT = 1e-4, 0.02            # sigma8 / sigma1 of the reference's 8 x 9 system; share of hypotheses the gate may leave out
F_MEASURED = 2.3e-9
F_BOUND = 10 * F_MEASURED
P3P_GATE, P3P_LEFT_OUT = 1e-4, 0.05        # root separation of the reference's quartic
REFINE_MEASURED = 3.0e-8                   # ONE case sets it (the planar 600-point problem, where the oracle's LM stops early); 7e-9 or less elsewhere
REFINE_BOUND = 10 * REFINE_MEASURED
# float32 inputs carry 6e-8 of relative rounding, a P3P triangle of these scenes (sides ~1 at depth ~2) amplifies it by up to ~1e3;
# the pose of another root of the quartic is 1e-2 or more away
TRUE_POSE_TOL = 1e-4

F_SIZES = (8, 9, 255, 256, 257, 513, 600)
P_SIZES = (4, 5, 255, 256, 257, 600)
RAGGED = (257, 9, 0, 600)
SEED = 11


# ------------------------------------------------------------------ inputs (made on the CPU; EXPERIMENTS.md has what the gates leave out of them)
def fm_cases():
    cases = {f"n{n}": fm_scene(n) for n in F_SIZES}
    cases["planar257"] = fm_scene(257, planar=True)
    return cases


def pnp_cases():
    cases = {f"n{n}": pnp_scene(n) for n in P_SIZES}
    cases["planar257"] = pnp_scene(257, planar=True)
    cases["exact257"] = pnp_scene(257, noise=0.0, outliers=0.0)
    cases["exact_planar257"] = pnp_scene(257, planar=True, noise=0.0, outliers=0.0)
    return cases


def bearings(uv, K4):
    b = np.c_[(uv[:, 0].astype(np.float64) - K4[2]) / K4[0], (uv[:, 1].astype(np.float64) - K4[3]) / K4[1], np.ones(len(uv))]
    return b / np.linalg.norm(b, axis=1)[:, None]


# ------------------------------------------------------------------ the hooks
def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class Stages:
    def __init__(self, L):
        self.L = L
        self.h = C.c_void_p()
        assert L.dvs_matcher_create(0, C.byref(self.h)) == 0

    def close(self):
        self.L.dvs_matcher_destroy(self.h)

    def fm(self, problems, seeds, H=H):
        nprob = len(problems)
        off = np.zeros(nprob + 1, np.int32); off[1:] = np.cumsum([len(p[0]) for p in problems])
        total = int(off[-1])
        p1 = np.ascontiguousarray(np.concatenate([p[0].reshape(-1, 2) for p in problems] + [np.zeros((1, 2), np.float32)]), np.float32)
        p2 = np.ascontiguousarray(np.concatenate([p[1].reshape(-1, 2) for p in problems] + [np.zeros((1, 2), np.float32)]), np.float32)
        sd = np.asarray(seeds, np.uint64)
        F = np.full((nprob, H, 9), np.nan); valid = np.full((nprob, H), -7, np.int32); counts = np.full((nprob, H), -7, np.int32)
        sel = np.full((nprob, 4), -7, np.int32); mask = np.full(total + 1, 9, np.uint8); Fb = np.full((nprob, 9), np.nan)
        rc = self.L.dvs_test_fm_stages(self.h, nprob, _p(off), _p(p1), _p(p2), THR_F, CONF, H, _p(sd), _p(F), _p(valid), _p(counts), _p(sel), _p(mask), _p(Fb))
        assert rc == 0, self.L.dvs_last_error()
        assert mask[total] == 9
        return [dict(F=F[b], valid=valid[b], counts=counts[b], sel=sel[b], mask=mask[off[b]:off[b + 1]], Fbest=Fb[b]) for b in range(nprob)]

    def pnp(self, problems, K4, seeds, H=H):
        nprob = len(problems)
        off = np.zeros(nprob + 1, np.int32); off[1:] = np.cumsum([len(p[0]) for p in problems])
        total = int(off[-1])
        X = np.ascontiguousarray(np.concatenate([p[0].reshape(-1, 3) for p in problems] + [np.zeros((1, 3), np.float32)]), np.float32)
        uv = np.ascontiguousarray(np.concatenate([p[1].reshape(-1, 2) for p in problems] + [np.zeros((1, 2), np.float32)]), np.float32)
        sd = np.asarray(seeds, np.uint64); K = np.ascontiguousarray(K4, np.float64)
        poses = np.full((nprob, 4 * H, 12), np.nan); valid = np.full((nprob, 4 * H), -7, np.int32); counts = np.full((nprob, 4 * H), -7, np.int32)
        sel = np.full((nprob, 4), -7, np.int32); inl = np.full(total + 1, -7, np.int32); nin = np.zeros(nprob, np.int32); ok = np.zeros(nprob, np.int32)
        rv = np.zeros((nprob, 3)); tv = np.zeros((nprob, 3))
        rc = self.L.dvs_test_pnp_stages(self.h, nprob, _p(off), _p(X), _p(uv), _p(K), THR_P, CONF, H, _p(sd), _p(poses), _p(valid), _p(counts), _p(sel),
                                        _p(inl), _p(nin), _p(ok), _p(rv), _p(tv))
        assert rc == 0, self.L.dvs_last_error()
        assert inl[total] == -7
        return [dict(poses=poses[b], valid=valid[b], counts=counts[b], sel=sel[b], inliers=inl[off[b]:off[b] + nin[b]], nin=int(nin[b]), ok=int(ok[b]),
                     rvec=rv[b], tvec=tv[b], tail=inl[off[b] + nin[b]:off[b + 1]]) for b in range(nprob)]

    def refine(self, X, uv, K4, pose, thr):
        X = np.ascontiguousarray(X, np.float32); uv = np.ascontiguousarray(uv, np.float32); K = np.ascontiguousarray(K4, np.float64)
        n = len(X); inl = np.full(n + 1, -7, np.int32); nin = np.full(1, -7, np.int32); ok = np.full(1, -7, np.int32)
        rv = np.full(3, np.nan); tv = np.full(3, np.nan)
        pose = None if pose is None else np.ascontiguousarray(pose, np.float64)
        rc = self.L.dvs_test_pnp_refine(_p(X), _p(uv), n, _p(K), None if pose is None else _p(pose), thr, _p(inl), _p(nin), _p(ok), _p(rv), _p(tv))
        assert rc == 0, self.L.dvs_last_error()
        assert inl[n] == -7
        return inl[:n], int(nin[0]), int(ok[0]), rv, tv

    def select(self, counts, n, model_points, group, confidence=CONF):
        c = np.ascontiguousarray(counts, np.int32); sel = np.full(4, -7, np.int32)
        rc = self.L.dvs_test_ransac_select(_p(c), len(c), n, model_points, confidence, group, _p(sel))
        assert rc == 0, self.L.dvs_last_error()
        return sel


@pytest.fixture(scope="module")
def stages(gpu, hooks):
    s = Stages(hooks)
    yield s
    s.close()


@pytest.fixture(scope="module")
def fm_runs(stages):
    """every fundamental-matrix input run ONCE through the stage hook: single problems, the all-identical problem, the ragged batch"""
    cases = fm_cases()
    runs = {k: (p, stages.fm([p], [SEED])[0]) for k, p in cases.items()}
    same = (np.full((20, 2), 7.0, np.float32), np.full((20, 2), 7.0, np.float32))
    runs["identical"] = (same, stages.fm([same], [SEED])[0])
    probs = [fm_scene(n, planar=(i == 3)) for i, n in enumerate(RAGGED)]
    seeds = [SEED + 5 * i for i in range(len(RAGGED))]
    for i, out in enumerate(stages.fm(probs, seeds)):
        runs[f"ragged{i}"] = (probs[i], out, seeds[i])
    runs["ragged_inputs"] = (probs, seeds)
    return runs


@pytest.fixture(scope="module")
def pnp_runs(stages):
    cases = pnp_cases()
    runs = {k: (c, stages.pnp([c[:2]], c[2], [SEED])[0], SEED) for k, c in cases.items()}
    probs = [pnp_scene(n, planar=(i == 3)) for i, n in enumerate(RAGGED)]
    seeds = [SEED + 5 * i for i in range(len(RAGGED))]
    for i, out in enumerate(stages.pnp([c[:2] for c in probs], probs[0][2], seeds)):
        runs[f"ragged{i}"] = (probs[i], out, seeds[i])
    runs["ragged_inputs"] = (probs, seeds)
    # n >= 4 and still nothing to select: no triangle of these points has a pose (one point twenty times; twenty points on a line)
    K4 = probs[0][2]
    uv = cases["n257"][1][:20]
    line = np.c_[0.5 * np.arange(20), np.zeros(20), np.full(20, 3.0)].astype(np.float32)
    degen = [(np.tile(np.float32([0.5, -0.25, 3.0]), (20, 1)), uv), (line, uv)]
    for i, out in enumerate(stages.pnp(degen, K4, [SEED, SEED + 1])):
        runs[f"degenerate{i}"] = out
    return runs


FM_KEYS = [f"n{n}" for n in F_SIZES] + ["planar257"] + [f"ragged{i}" for i in range(len(RAGGED))]
PNP_KEYS = [f"n{n}" for n in P_SIZES] + ["planar257"] + [f"ragged{i}" for i in range(len(RAGGED))]


def _fm(fm_runs, key):
    r = fm_runs[key]
    return r[0][0], r[0][1], r[1], (r[2] if len(r) > 2 else SEED)


def band_count(e, thr):
    """(#{e <= thr^2 (1 - BAND)}, #{e <= thr^2 (1 + BAND)}) of an error vector (rows: hypotheses)"""
    t2 = thr * thr
    return (e <= t2 * (1 - BAND)).sum(-1), (e <= t2 * (1 + BAND)).sum(-1)


# ------------------------------------------------------------------ fundamental matrix: sampler and hypotheses
@pytest.mark.parametrize("key", FM_KEYS)
def test_f_hypotheses(fm_runs, oracle, key):
    p1, p2, out, seed = _fm(fm_runs, key)
    n = len(p1)
    if n < 8:
        assert (out["valid"] == 0).all()
        return
    left_out, worst, worst_refs = 0, 0.0, 0.0
    for h in range(H):
        idx = ref.sample(seed, h, n, 8)
        Fr, ratio = ref.eight_point(p1[idx], p2[idx])
        assert out["valid"][h] == 1 and Fr is not None, h                             # every sample of generic points is valid, in both
        F = out["F"][h].reshape(3, 3)
        assert abs(np.linalg.norm(F) - 1) < 1e-12 and abs(np.linalg.det(F)) < 1e-9, h
        if ratio < F_GATE:
            left_out += 1
            continue
        worst = max(worst, min(np.abs(F - Fr).max(), np.abs(F + Fr).max()))
        Fo = oracle.eight_point(p1[idx], p2[idx])
        worst_refs = max(worst_refs, min(np.abs(Fo - Fr).max(), np.abs(Fo + Fr).max()))
    print(f"{key}: left out {left_out} / {H}, kernel - reference {worst:.3e}, oracle - reference {worst_refs:.3e}, bound {F_BOUND:.1e}")
    assert F_BOUND < 1e-6
    assert left_out <= F_LEFT_OUT * H
    assert worst_refs <= F_MEASURED, "the two references disagree by more than the measured figure: the bound's provenance is stale"
    assert worst <= F_BOUND


def test_f_identical_points_have_no_valid_hypothesis(fm_runs):
    (p1, p2), out = fm_runs["identical"]
    assert ref.eight_point(p1[:8], p2[:8])[0] is None
    assert (out["valid"] == 0).all() and (out["F"] == 0).all() and (out["counts"] == 0).all()
    assert out["sel"][0] == -1 and out["sel"][2] == 0 and (out["mask"] == 0).all() and (out["Fbest"] == 0).all()


# ------------------------------------------------------------------ score, select, mask
@pytest.mark.parametrize("key", FM_KEYS)
def test_f_score_select_mask(fm_runs, key):
    p1, p2, out, seed = _fm(fm_runs, key)
    n = len(p1)
    if n < 8:
        assert (out["counts"] == 0).all() and out["sel"][0] == -1 and out["sel"][2] == 0 and (out["mask"] == 0).all() and (out["Fbest"] == 0).all()
        return
    e = np.stack([ref.epipolar_error(out["F"][h], p1, p2) for h in range(H)])
    lo, hi = band_count(e, THR_F)
    assert (lo == hi).all(), "a point of the input lies inside the band: choose another scene"
    assert (out["counts"] == np.where(out["valid"] == 1, lo, 0)).all(), np.flatnonzero(out["counts"] != lo)
    best, it, cnt, margin = ref.replay_select(out["counts"], n, 8, CONF, 1)
    assert margin > 1e-6
    assert tuple(out["sel"][:3]) == (best, it, cnt)
    if best < 0:                                                                       # (n = 8: the one sample's rank-2 model does not hold all eight)
        assert key == "n8" and (out["mask"] == 0).all() and (out["Fbest"] == 0).all()
        return
    assert (out["mask"] == (e[best] <= THR_F * THR_F)).all()
    assert out["mask"].sum() == out["sel"][2]
    assert out["Fbest"].tobytes() == out["F"][best].tobytes()


def test_f_hooks_equal_the_product_calls(fm_runs):
    from dvslam_amd import FrontendGlue
    g = FrontendGlue()
    probs, seeds = fm_runs["ragged_inputs"]
    batch = g.find_fundamental_ransac_batch([p[0] for p in probs], [p[1] for p in probs], seeds, THR_F, CONF, H)
    for i in range(len(probs)):
        out = fm_runs[f"ragged{i}"][1]
        assert (batch[i][0] == out["mask"]).all() and batch[i][1] == out["sel"][2], i
    # the batch's F9 (the glue passes none): the C entry point itself, every problem but the first at a non-zero offset and index
    off = np.zeros(len(probs) + 1, np.int32); off[1:] = np.cumsum([len(p[0]) for p in probs])
    p1 = np.ascontiguousarray(np.concatenate([p[0] for p in probs]), np.float32); p2 = np.ascontiguousarray(np.concatenate([p[1] for p in probs]), np.float32)
    sd = np.asarray(seeds, np.uint64); F9 = np.full((len(probs), 9), np.nan); mask = np.full(int(off[-1]), 9, np.uint8); nin = np.full(len(probs), -7, np.int32)
    assert g._L.dvs_find_fundamental_ransac_batch(g._h, len(probs), _p(off), _p(p1), _p(p2), THR_F, CONF, H, _p(sd), _p(F9), _p(mask), _p(nin)) == 0
    for i in range(len(probs)):
        out = fm_runs[f"ragged{i}"][1]
        assert F9[i].tobytes() == out["Fbest"].tobytes() and (mask[off[i]:off[i + 1]] == out["mask"]).all() and nin[i] == out["sel"][2], i
    assert any(F9[i].any() for i in range(1, len(probs)))
    for key in ("n9", "n600"):
        (p1, p2), out = fm_runs[key]
        F, mask, nin = g.find_fundamental_ransac(p1, p2, THR_F, CONF, H, seed=SEED)
        assert (mask == out["mask"]).all() and nin == out["sel"][2] and F.tobytes() == out["Fbest"].tobytes(), key
    g.close()


@pytest.mark.parametrize("case", ref.SELECT_CASES, ids=[c["name"] for c in ref.SELECT_CASES])
def test_select_on_hand_made_counts(stages, case):
    want = ref.replay_select(case["counts"], ref.SELECT_N, case["model_points"], ref.SELECT_CONFIDENCE, case["group"])
    assert want[:3] == case["expect"] and want[3] > 1e-6
    sel = stages.select(case["counts"], ref.SELECT_N, case["model_points"], case["group"], ref.SELECT_CONFIDENCE)
    assert tuple(sel[:3]) == case["expect"] and sel[3] == 0


# ------------------------------------------------------------------ PnP: P3P hypotheses
def _pnp(pnp_runs, key):
    (X, uv, K4, behind, R, t), out, seed = pnp_runs[key]
    return X, uv, K4, behind, R, t, out, seed


def _check_p3p(X, uv, K4, out, seed):
    n = len(X)
    valid = out["valid"].reshape(H, 4); poses = out["poses"].reshape(H, 4, 12)
    if n < 4:
        assert (valid == 0).all()
        return
    j = bearings(uv, K4)
    left_out = 0
    for h in range(H):
        idx = ref.sample(seed, h, n, 3)
        nv = int(valid[h].sum())
        assert (valid[h][:nv] == 1).all() and (valid[h][nv:] == 0).all(), h          # a prefix of the four slots
        vs = []
        for s in range(nv):
            R = poses[h, s, :9].reshape(3, 3); t = poses[h, s, 9:]
            assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-9 and np.linalg.det(R) > 0, (h, s)
            Xc = X[idx].astype(np.float64) @ R.T + t
            vs.append(np.linalg.norm(Xc[2]) / np.linalg.norm(Xc[0]))
        sols, sep = ref.p3p_roots(X[idx], j[idx])
        if sep < P3P_GATE:
            left_out += 1
            continue
        assert nv == len(sols), (h, nv, sols, sep)
        assert all(b > a for a, b in zip(vs, vs[1:])), (h, vs)
        # the same roots: a root moves by the coefficients' rounding (1e-13 after the cancellations of either derivation) over the separation
        assert np.allclose(vs, [v for v, u in sols], rtol=1e-9 / sep, atol=0), (h, vs, sols)
        for s in range(nv):
            e = ref.reprojection_error2(poses[h, s, :9], poses[h, s, 9:], K4, X[idx], uv[idx])
            assert np.sqrt(e).max() < 1e-6, (h, s, e)
    print(f"left out {left_out} / {H}")
    assert left_out <= P3P_LEFT_OUT * H


@pytest.mark.parametrize("key", PNP_KEYS)
def test_p3p_hypotheses(pnp_runs, key):
    X, uv, K4, behind, R, t, out, seed = _pnp(pnp_runs, key)
    _check_p3p(X, uv, K4, out, seed)


@pytest.mark.parametrize("key", ["exact257", "exact_planar257"])
def test_p3p_finds_the_true_pose_on_exact_scenes(pnp_runs, key):
    """noise-free scenes, the fronto-parallel planar one included (double roots): the true pose is among the poses of >= 97 % of the samples
    that do not hold a point moved behind the camera (the bar tests/test_ransac.py sets for the same routine on the host).

    Sample 181 of exact_planar257 (points 87, 251, 243; quartic roots 3.0e-4 apart, inside the 1e-4 gate) is the one that showed that a
    root of the quartic alone is not enough: its poses were 3.8e-6 and 4.2e-6 px off their third sample point until p3p_solve began to
    polish (u, v) on the two cosine laws."""
    X, uv, K4, behind, R, t, out, seed = _pnp(pnp_runs, key)
    _check_p3p(X, uv, K4, out, seed)                                                  # the general properties hold here too
    valid = out["valid"].reshape(H, 4); poses = out["poses"].reshape(H, 4, 12)
    clean = [h for h in range(H) if not set(ref.sample(seed, h, len(X), 3)) & set(behind.tolist())]
    found = sum(any(np.abs(poses[h, s, :9].reshape(3, 3) - R).max() + np.abs(poses[h, s, 9:] - t).max() < TRUE_POSE_TOL for s in range(4) if valid[h, s])
                for h in clean)
    print(f"{key}: true pose among the poses of {found} / {len(clean)} samples")
    assert len(clean) > 0.8 * H and found >= 0.97 * len(clean)


# ------------------------------------------------------------------ PnP: score, select, inlier list, refinement
def _rt_residuals(x, X, uv, K4):
    Xc = X @ rs.rodrigues_to_R(x[:3]).T + x[3:]
    return np.concatenate([K4[0] * Xc[:, 0] / Xc[:, 2] + K4[2] - uv[:, 0], K4[1] * Xc[:, 1] / Xc[:, 2] + K4[3] - uv[:, 1]])


@pytest.mark.parametrize("key", PNP_KEYS)
def test_pnp_score_select_inliers_refine(pnp_runs, key):
    X, uv, K4, behind, R, t, out, seed = _pnp(pnp_runs, key)
    n = len(X)
    if n < 4:
        assert (out["counts"] == 0).all() and out["sel"][0] == -1 and out["nin"] == 0 and out["ok"] == 0
        assert (out["rvec"] == 0).all() and (out["tvec"] == 0).all()
        return
    H4 = 4 * H
    e = np.stack([ref.reprojection_error2(out["poses"][h, :9], out["poses"][h, 9:], K4, X, uv) if out["valid"][h] else np.full(n, np.inf) for h in range(H4)])
    lo, hi = band_count(e, THR_P)
    assert (lo == hi).all(), "a point of the input lies inside the band: choose another scene"
    assert (out["counts"] == lo).all(), np.flatnonzero(out["counts"] != lo)           # invalid slots: 0
    best, it, cnt, margin = ref.replay_select(out["counts"], n, 3, CONF, 4)
    assert margin > 1e-6
    assert tuple(out["sel"][:3]) == (best, it, cnt)
    assert best >= 0 and out["ok"] == 1
    want = np.flatnonzero(e[best] <= THR_P * THR_P)
    assert out["inliers"].tolist() == want.tolist() and out["nin"] == out["sel"][2] == len(want)
    assert (out["tail"] == -7).all()                                                   # nothing written behind the list
    if n >= 255:                                                                       # behind the camera: never an inlier, though on the pixel —
        assert len(behind) and not set(want.tolist()) & set(behind.tolist())           # only the depth test keeps these points out
        Xc = X[behind].astype(np.float64) @ R.T + t     # (the TRUE pose: a minimal-sample pose's rotation and translation errors cancel in front only)
        du = K4[0] * Xc[:, 0] / Xc[:, 2] + K4[2] - uv[behind, 0]; dv = K4[1] * Xc[:, 1] / Xc[:, 2] + K4[3] - uv[behind, 1]
        assert (Xc[:, 2] < 0).all() and (du * du + dv * dv <= THR_P * THR_P).all()
    # refinement
    least_squares = pytest.importorskip("scipy.optimize").least_squares
    Xi = X[want].astype(np.float64); uvi = uv[want].astype(np.float64)
    Rb = out["poses"][best, :9].reshape(3, 3); tb = out["poses"][best, 9:]
    x0 = np.concatenate([ref.rodrigues(Rb), tb])
    xk = np.concatenate([out["rvec"], out["tvec"]])
    c0 = (_rt_residuals(x0, Xi, uvi, K4) ** 2).sum(); ck = (_rt_residuals(xk, Xi, uvi, K4) ** 2).sum()
    assert ck <= c0 * (1 + 1e-12)
    assert np.linalg.norm(out["rvec"]) <= math.pi
    if len(want) >= 4:                                                                 # (3 points: 6 residuals for 6 unknowns, a root not a minimum)
        sol = least_squares(_rt_residuals, x0, args=(Xi, uvi, K4), method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15)
        d = np.abs(sol.x - xk).max()
        print(f"{key}: {len(want)} inliers, cost {c0:.6f} -> {ck:.6f} (scipy {2 * sol.cost:.6f}), kernel - scipy {d:.3e}, bound {REFINE_BOUND:.1e}")
        assert d <= REFINE_BOUND


@pytest.mark.parametrize("key", ["degenerate0", "degenerate1"])
def test_pnp_nothing_selected_gives_all_zeros(pnp_runs, key):
    """20 points of which no three span a triangle: P3P has no pose, every count is 0, select ends at best = -1 after all H iterations, the
    refinement returns at once"""
    out = pnp_runs[key]
    assert (out["valid"] == 0).all() and (out["counts"] == 0).all()
    assert tuple(out["sel"][:3]) == (-1, H, 0)
    assert out["nin"] == 0 and out["ok"] == 0 and (out["rvec"] == 0).all() and (out["tvec"] == 0).all()
    assert (out["tail"] == -7).all()                                                   # no inlier index written


@pytest.mark.parametrize("m", [0, 1, 2])
def test_pnp_refine_leaves_the_pose_with_fewer_than_three_inliers(stages, m):
    """k_pnp_refine alone (dvs_test_pnp_refine): select never hands it a pose with fewer than 3 inliers, so the estimator cannot show this.
    Six noise-free points under their true pose, all but the first m moved 50 px off: m inliers, no LM step, the pose comes back as
    given (t bit for bit, the rotation through the Rodrigues vector within 1e-9)."""
    X, uv, K4, behind, R, t = pnp_scene(257, noise=0.0, outliers=0.0)
    keep = [i for i in range(20) if i not in set(behind.tolist())][:6]
    X = X[keep]; uv = uv[keep].copy(); uv[m:] += np.float32(50.0)
    e = np.sqrt(ref.reprojection_error2(R.reshape(-1), t, K4, X, uv))
    assert (e[:m] < 0.01).all() and (e[m:] > 40).all()
    inl, nin, ok, rv, tv = stages.refine(X, uv, K4, np.concatenate([R.reshape(-1), t]), THR_P)
    assert nin == m and inl[:m].tolist() == list(range(m)) and (inl[m:] == -1).all()
    assert ok == (1 if m > 0 else 0)
    assert tv.tobytes() == np.asarray(t, np.float64).tobytes()
    assert np.abs(rs.rodrigues_to_R(rv) - R).max() <= 1e-9


def test_pnp_refine_with_nothing_selected(stages):
    X, uv, K4, behind, R, t = pnp_scene(5, noise=0.0, outliers=0.0)
    inl, nin, ok, rv, tv = stages.refine(X, uv, K4, None, THR_P)
    assert nin == 0 and ok == 0 and (rv == 0).all() and (tv == 0).all() and (inl == -1).all()


def test_pnp_hooks_equal_the_product_calls(pnp_runs):
    from dvslam_amd import FrontendGlue
    g = FrontendGlue()
    probs, seeds = pnp_runs["ragged_inputs"]
    batch = g.solve_pnp_ransac_batch([p[0] for p in probs], [p[1] for p in probs], probs[0][2], seeds, H, THR_P, CONF)
    for i in range(len(probs)):
        out = pnp_runs[f"ragged{i}"][1]
        assert bool(batch[i][0]) == bool(out["ok"]) and batch[i][3].tolist() == out["inliers"].tolist(), i
        assert batch[i][1].tobytes() == out["rvec"].tobytes() and batch[i][2].tobytes() == out["tvec"].tobytes(), i
    g.close()
