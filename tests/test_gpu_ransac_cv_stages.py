"""The OpenCV-procedure robust estimators (csrc/ransac.hip, csrc/pnp_cv.h: dvs_find_fundamental_cv*, dvs_solve_pnp_ransac_cv*) STAGE BY STAGE
against the float64 statements of tests/ransac_cv_stage_ref.py.  tests/test_ransac.py compares the whole estimators with the CPU oracle at
the end, which RANSAC — and the 20 Levenberg-Marquardt iterations of the refit — pass with a broken stage.  Here every stage gets the
GPU's own output of the stage before it (include/dvslam_hip_test_ransac_cv.h) and is compared exactly, or to a bound with a stated
provenance.  Every *_MEASURED figure is a difference between TWO float64 statements neither of which is the kernel, measured on the CPU
by tests/test_ransac_cv_stage_ref_cpu.py (which asserts it) and recorded in EXPERIMENTS.md, "RANSAC stage tests, OpenCV procedure"; the
kernel gets ten times the figure.

The EPnP hypotheses have no such bound: ref.epnp5 and the oracle's EPnP (and the kernel's) differ by the SIGNS their eigen-decompositions
give the control points' axes, on which the pose of a sample without an exact rigid solution depends, and on noise-free samples the gate
on the three reprojection errors leaves nothing to compare (EXPERIMENTS.md has the figures).  They are held to the truth on the noise-free
case and to what the algorithm defines on every case."""
import ctypes as C
import numpy as np
import pytest
import ransac_cv_stage_ref as ref
import ransac_scenes as rs
from ransac_stage_ref import rodrigues

pytestmark = pytest.mark.gpu

H = 100
THR_F, THR_P, CONF = 2.0, 4.0, 0.99
# 7-point models: ref.seven_point (SVD null space, interpolated cubic, np.roots) against oracle.seven_point (Jacobi eigenvectors of A^T A,
# closed-form cubic), matched as sets at unit norm, over the gated samples (sigma7 / sigma1 and root separation above F7_GATE) of the
# cases n = 15, 16, 255, 256, 257, 513, 600 and planar 257 (100 samples each) and of the LMedS scenes n = 8, 9, 11, 13, 14 (300 each):
# 7.13e-9 (LMedS 14; 2.49e-9 planar 257, 1.5e-9 or less elsewhere).  The gate leaves out no sample.
F7_GATE, F7_LEFT_OUT = 1e-7, 0.05
F7_MEASURED = 7.2e-9
F7_BOUND = 10 * F7_MEASURED
# refit initialisation: ref.refit_init (SVD of the DLT system itself, polar factor by SVD) against the initialisation of
# oracle/pnp_cv_oracle.cpp (Jacobi eigenvectors of the normal matrix), rvec and tvec entries, on the oracle estimator's inlier sets of the
# non-planar cases n = 63 .. 600 and noise-free 257 (DLT) and on the planar inlier sets of 65 and 257 points, noisy and noise-free
# (homography): 6.384e-15.  The oracle's planar initialisation, like the kernel's, omits cv::findHomography's Levenberg-Marquardt polish, and
# ref.refit_init omits it too: the three state the same thing.  (The estimator's inlier sets of the PLANAR cases hold the points moved
# behind the camera, which the float error measure cannot tell from inliers: nearly planar, DLT, not a defined initialisation — left out.)
INIT_MEASURED = 6.4e-15
INIT_BOUND = 10 * INIT_MEASURED
# refit: oracle.solve_pnp_iterative (CvLevMarq: stops on a relative step below FLT_EPSILON or after 20 iterations) against
# ref.refit_optimum (scipy, tolerances 1e-15) from ref.refit_init's start, on the oracle estimator's inlier sets of every PnP case:
# 1.13e-8 (planar 257; 4.2e-9 planar 65, 2.2e-10 or less on the others) — how far that stop leaves the pose from the optimum
REFIT_MEASURED = 1.2e-8
REFIT_BOUND = 10 * REFIT_MEASURED
# float32 inputs carry 6e-8 of relative rounding; a 5-point EPnP sample of these scenes amplifies it by up to ~1e3 (as a P3P triangle does)
TRUE_POSE_TOL = 1e-4
BAND_CAP = 3                                # in-band points of a whole case: more and the case is inconclusive — choose another seed

F_SIZES = (15, 16, 255, 256, 257, 513, 600)
L_SIZES = (8, 9, 13, 14)
P_SIZES = (6, 7, 63, 64, 65, 255, 256, 257, 600)
H_VALUES = (1, 3, 4, 5, 63, 64, 65, 100)
RAGGED_F = (257, 15, 600, 16)
RAGGED_L = (14, 8, 11)
RAGGED_P = (257, 5, 0, 600, 6)
LMEDS_ITERS = 300                           # RANSACUpdateNumIters(0.99, 0.45, 7, .) = ln(0.01) / ln(1 - 0.55^7) = 300.2


def fm_cases():
    cases = {f"n{n}": rs.fm_scene(n) for n in F_SIZES}
    cases["planar257"] = rs.fm_scene(257, planar=True)
    return cases


def pnp_cases():
    cases = {f"n{n}": rs.pnp_scene(n) for n in P_SIZES}
    cases["planar65"] = rs.pnp_scene(65, planar=True)
    cases["planar257"] = rs.pnp_scene(257, planar=True)
    cases["exact257"] = rs.pnp_scene(257, noise=0.0, outliers=0.0)
    cases["exact_planar257"] = rs.pnp_scene(257, planar=True, noise=0.0, outliers=0.0)
    return cases


def ragged_pnp():
    return [rs.pnp_scene(n, planar=(i == 3)) for i, n in enumerate(RAGGED_P)]


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

    def fm(self, problems, H=H, max_iters=1000):
        nprob = len(problems)
        off = np.zeros(nprob + 1, np.int32); off[1:] = np.cumsum([len(p[0]) for p in problems])
        total = int(off[-1])
        p1 = np.ascontiguousarray(np.concatenate([p[0].reshape(-1, 2) for p in problems] + [np.zeros((1, 2), np.float32)]), np.float32)
        p2 = np.ascontiguousarray(np.concatenate([p[1].reshape(-1, 2) for p in problems] + [np.zeros((1, 2), np.float32)]), np.float32)
        smp = np.full((nprob, H, 7), -7, np.int32); found = np.full(nprob, -7, np.int32)
        F = np.full((nprob, 3 * H, 9), np.nan); valid = np.full((nprob, 3 * H), -7, np.int32); counts = np.full((nprob, 3 * H), -7, np.int32)
        sel = np.full((nprob, 4), -7, np.int32); mask = np.full(total + 1, 9, np.uint8); Fb = np.full((nprob, 9), np.nan)
        rc = self.L.dvs_test_fm_cv_stages(self.h, nprob, _p(off), _p(p1), _p(p2), THR_F, CONF, max_iters, H, _p(smp), _p(found), _p(F), _p(valid),
                                          _p(counts), _p(sel), _p(mask), _p(Fb))
        assert rc == 0, self.L.dvs_last_error()
        assert mask[total] == 9
        return [dict(samples=smp[b], found=int(found[b]), F=F[b], valid=valid[b], counts=counts[b], sel=sel[b], mask=mask[off[b]:off[b + 1]].copy(),
                     Fbest=Fb[b]) for b in range(nprob)]

    def pnp(self, problems, K4, H=H):
        nprob = len(problems)
        off = np.zeros(nprob + 1, np.int32); off[1:] = np.cumsum([len(p[0]) for p in problems])
        total = int(off[-1])
        X = np.ascontiguousarray(np.concatenate([p[0].reshape(-1, 3) for p in problems] + [np.zeros((1, 3), np.float32)]), np.float32)
        uv = np.ascontiguousarray(np.concatenate([p[1].reshape(-1, 2) for p in problems] + [np.zeros((1, 2), np.float32)]), np.float32)
        K = np.ascontiguousarray(K4, np.float64)
        smp = np.full((nprob, H, 5), -7, np.int32); models = np.full((nprob, H, 18), np.nan); counts = np.full((nprob, H), -7, np.int32)
        sel = np.full((nprob, 4), -7, np.int32); inl = np.full(total + 1, -7, np.int32); nin = np.full(nprob, -7, np.int32); ok = np.full(nprob, -7, np.int32)
        rv = np.full((nprob, 3), np.nan); tv = np.full((nprob, 3), np.nan)
        rc = self.L.dvs_test_pnp_cv_stages(self.h, nprob, _p(off), _p(X), _p(uv), _p(K), THR_P, CONF, H, _p(smp), _p(models), _p(counts), _p(sel), _p(inl),
                                           _p(nin), _p(ok), _p(rv), _p(tv))
        assert rc == 0, self.L.dvs_last_error()
        assert inl[total] == -7
        return [dict(samples=smp[b], models=models[b], counts=counts[b], sel=sel[b], inliers=inl[off[b]:off[b] + nin[b]].copy(), nin=int(nin[b]), ok=int(ok[b]),
                     rvec=rv[b], tvec=tv[b], tail=inl[off[b] + nin[b]:off[b + 1]].copy()) for b in range(nprob)]

    def select(self, counts, n, model_points, group, found, max_iters, confidence=CONF):
        c = np.ascontiguousarray(counts, np.int32); sel = np.full(4, -7, np.int32)
        rc = self.L.dvs_test_ransac_select_cv(_p(c), len(c), n, model_points, confidence, group, found, max_iters, _p(sel))
        assert rc == 0, self.L.dvs_last_error()
        return sel

    def refit(self, X, uv, K4, model6, thr=THR_P):
        X = np.ascontiguousarray(X, np.float32); uv = np.ascontiguousarray(uv, np.float32); K = np.ascontiguousarray(K4, np.float64)
        n = len(X); inl = np.full(n + 1, -7, np.int32); nin = np.full(1, -7, np.int32); ok = np.full(1, -7, np.int32)
        rv = np.full(3, np.nan); tv = np.full(3, np.nan); dbg = np.full(8, np.nan)
        m6 = None if model6 is None else np.ascontiguousarray(model6, np.float64)
        rc = self.L.dvs_test_pnpcv_refit(_p(X), _p(uv), n, _p(K), None if m6 is None else _p(m6), thr, _p(inl), _p(nin), _p(ok), _p(rv), _p(tv), _p(dbg))
        assert rc == 0, self.L.dvs_last_error()
        assert inl[n] == -7
        return dict(inliers=inl[:n], nin=int(nin[0]), ok=int(ok[0]), rvec=rv, tvec=tv, init=dbg[:6].copy(), path=int(dbg[6]), iters=int(dbg[7]))


@pytest.fixture(scope="module")
def stages(gpu, hooks):
    s = Stages(hooks)
    yield s
    s.close()


@pytest.fixture(scope="module")
def fm_runs(stages):
    """every fundamental-matrix input run ONCE through the stage hook: single problems and the ragged batch"""
    runs = {k: (p, stages.fm([p])[0]) for k, p in fm_cases().items()}
    probs = [rs.fm_scene(n) for n in RAGGED_F]
    for i, out in enumerate(stages.fm(probs)):
        runs[f"ragged{i}"] = (probs[i], out)
    return runs


@pytest.fixture(scope="module")
def lmeds_runs(stages):
    runs = {f"n{n}": (rs.lmeds_scene(n), stages.fm([rs.lmeds_scene(n)], H=LMEDS_ITERS)[0]) for n in L_SIZES}
    probs = [rs.lmeds_scene(n) for n in RAGGED_L]
    for i, out in enumerate(stages.fm(probs, H=LMEDS_ITERS)):
        runs[f"ragged{i}"] = (probs[i], out)
    return runs


@pytest.fixture(scope="module")
def pnp_runs(stages):
    runs = {k: (c, stages.pnp([c[:2]], c[2])[0]) for k, c in pnp_cases().items()}
    probs = ragged_pnp()
    for i, out in enumerate(stages.pnp([c[:2] for c in probs], probs[0][2])):
        runs[f"ragged{i}"] = (probs[i], out)
    return runs


FM_KEYS = [f"n{n}" for n in F_SIZES] + ["planar257"] + [f"ragged{i}" for i in range(len(RAGGED_F))]
LMEDS_KEYS = [f"n{n}" for n in L_SIZES] + [f"ragged{i}" for i in range(len(RAGGED_L))]
PNP_KEYS = [f"n{n}" for n in P_SIZES] + ["planar65", "planar257", "exact257", "exact_planar257"] + [f"ragged{i}" for i in range(len(RAGGED_P))]


def _same(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a)


# ------------------------------------------------------------------ fundamental matrix: samples and 7-point hypotheses
def check_f7(p1, p2, out, Hn):
    from dvslam_amd import glue
    n = len(p1)
    idx, found = glue.cv_ransac_subsets(p1, p2, 7, Hn)
    assert out["found"] == found and out["samples"][:found].tolist() == idx.tolist() and (out["samples"][found:] == 0).all()
    F = out["F"].reshape(Hn, 3, 9); valid = out["valid"].reshape(Hn, 3)
    assert (valid[found:] == 0).all() and (F[found:] == 0).all()
    x1 = np.c_[p1.astype(np.float64), np.ones(n)]; x2 = np.c_[p2.astype(np.float64), np.ones(n)]
    left_out, worst = 0, 0.0
    for h in range(found):
        nv = int(valid[h].sum())
        assert (valid[h][:nv] == 1).all() and (valid[h][nv:] == 0).all() and (F[h, nv:] == 0).all(), h     # the roots fill a prefix of the three slots
        for k in range(nv):
            Fk = F[h, k].reshape(3, 3)
            assert Fk[2, 2] == 1.0 or Fk[2, 2] == 0.0, (h, k)
            assert abs(np.linalg.det(Fk / np.linalg.norm(Fk))) < 1e-9, (h, k)
            a, b = x1[idx[h]], x2[idx[h]]
            r = np.abs(np.einsum("ni,ij,nj->n", b, Fk, a)) / (np.linalg.norm(Fk) * np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))
            assert r.max() < 1e-6, (h, k, r.max())
        models, ratio, sep = ref.seven_point(p1, p2, idx[h])
        if ratio < F7_GATE or sep < F7_GATE:
            left_out += 1
            continue
        assert nv == len(models), (h, nv, len(models), sep)
        worst = max(worst, ref.match_sets([F[h, k] for k in range(nv)], models))
    print(f"left out {left_out} / {found}, kernel - reference {worst:.3e}, bound {F7_BOUND:.1e}")
    assert left_out <= F7_LEFT_OUT * found
    assert worst <= F7_BOUND


@pytest.mark.parametrize("key", FM_KEYS)
def test_f7_samples_and_hypotheses(fm_runs, key):
    (p1, p2), out = fm_runs[key]
    check_f7(p1, p2, out, H)


@pytest.mark.parametrize("key", LMEDS_KEYS)
def test_f7_samples_and_hypotheses_below_fifteen_points(lmeds_runs, key):
    (p1, p2), out = lmeds_runs[key]
    check_f7(p1, p2, out, LMEDS_ITERS)


# ------------------------------------------------------------------ fundamental matrix: score, select, mask
def float_errors_f(out, p1, p2):
    with np.errstate(all="ignore"):
        return np.stack([ref.epipolar_error(F, p1, p2) if v else np.full(len(p1), np.inf) for F, v in zip(out["F"], out["valid"])])


def check_counts(counts, e, thr2):
    """counts[h] in [strict, strict + in band] of the reference's errors; the in-band points of the whole case number at most BAND_CAP"""
    sb = np.array([ref.count_float(row, thr2) for row in e])
    assert sb[:, 1].sum() <= BAND_CAP, "too many errors within rounding of the threshold: inconclusive, choose another seed"
    bad = np.flatnonzero((counts < sb[:, 0]) | (counts > sb[:, 0] + sb[:, 1]))
    assert len(bad) == 0, (bad[:5], counts[bad[:5]], sb[bad[:5]])


def check_mask(mask, e, thr2):
    t = float(thr2)
    sure_in = e < t * (1 - ref.BAND_F); sure_out = e > t * (1 + ref.BAND_F)
    assert (mask[sure_in] == 1).all() and (mask[sure_out] == 0).all()
    assert set(np.unique(mask).tolist()) <= {0, 1}


@pytest.mark.parametrize("key", FM_KEYS)
def test_f_score_select_mask(fm_runs, key):
    (p1, p2), out = fm_runs[key]
    n = len(p1)
    thr2 = float(np.float32(THR_F * THR_F))
    e = float_errors_f(out, p1, p2)
    assert (out["counts"][out["valid"] == 0] == 0).all()
    check_counts(out["counts"], e, thr2)
    best, it, cnt, more, margin = ref.replay_select_cv(out["counts"], n, 7, CONF, 3, out["found"], 1000)
    assert margin > 1e-6
    assert tuple(out["sel"]) == (best, it, cnt, more)
    assert best >= 0
    assert out["Fbest"].tobytes() == out["F"][best].tobytes()
    check_mask(out["mask"], e[best], thr2)
    assert out["mask"].sum() == out["sel"][2]


@pytest.mark.parametrize("case", ref.SELECT_CV_CASES, ids=[c["name"] for c in ref.SELECT_CV_CASES])
def test_select_cv_on_hand_made_counts(stages, case):
    want = ref.replay_select_cv(case["counts"], ref.SELECT_CV_N, case["model_points"], ref.SELECT_CV_CONFIDENCE, case["group"], case["found"], case["max_iters"])
    assert want[:4] == case["expect"] and want[4] > 1e-6
    sel = stages.select(case["counts"], ref.SELECT_CV_N, case["model_points"], case["group"], case["found"], case["max_iters"], ref.SELECT_CV_CONFIDENCE)
    assert tuple(sel) == case["expect"]


def test_nothing_selected_gives_zeros(stages):
    """15 points on a line in both images: getSubset finds no sample (every one is collinear), so no model, no count; sel[0] = -1, a mask
    and an Fbest of zeros"""
    t = np.arange(15, dtype=np.float32)
    p = np.stack([10 + 3 * t, 20 + 5 * t], 1)
    out = stages.fm([(p, p + np.float32(3))], H=4)[0]
    assert out["found"] == 0 and (out["valid"] == 0).all() and (out["counts"] == 0).all() and (out["F"] == 0).all()
    assert tuple(out["sel"]) == (-1, 0, 0, 0) and (out["mask"] == 0).all() and (out["Fbest"] == 0).all()


# ------------------------------------------------------------------ two passes are one pass
def test_two_passes_are_one_pass(stages):
    from dvslam_amd import FrontendGlue
    g = FrontendGlue()
    long_p, short_p = rs.loop_scene(0.5), rs.loop_scene(0.1)
    first = stages.fm([long_p], H=96)[0]
    full = stages.fm([long_p], H=1000)[0]
    assert first["sel"][3] == 1 and first["sel"][1] == 96
    assert full["sel"][3] == 0 and 96 < full["sel"][1] < 1000, full["sel"]
    assert full["samples"][:96].tobytes() == first["samples"].tobytes() and full["F"][:288].tobytes() == first["F"].tobytes()   # a prefix of the same sequence
    F, mask, nin, its = g.find_fundamental_cv(long_p[0], long_p[1], THR_F, CONF, 1000)
    assert F.tobytes() == full["Fbest"].tobytes() and (mask == full["mask"]).all() and nin == full["sel"][2] and its == full["sel"][1]
    early = stages.fm([short_p], H=96)[0]
    assert early["sel"][3] == 0 and early["sel"][1] < 96
    Fs, masks, nins, itss = g.find_fundamental_cv(short_p[0], short_p[1], THR_F, CONF, 1000)
    assert Fs.tobytes() == early["Fbest"].tobytes() and (masks == early["mask"]).all() and nins == early["sel"][2] and itss == early["sel"][1]
    batch = g.find_fundamental_cv_batch([long_p[0], short_p[0]], [long_p[1], short_p[1]], THR_F, CONF, 1000)
    assert (batch[0][0] == mask).all() and batch[0][1:] == (nin, its)
    assert (batch[1][0] == masks).all() and batch[1][1:] == (nins, itss)
    # the batch's F9 (the glue passes none): the C entry point itself, the second pass's F scattered over the first's — in both orders
    for order in ((long_p, short_p), (short_p, long_p)):
        off = np.array([0, 600, 1200], np.int32)
        p1 = np.ascontiguousarray(np.concatenate([order[0][0], order[1][0]]), np.float32); p2 = np.ascontiguousarray(np.concatenate([order[0][1], order[1][1]]), np.float32)
        F9 = np.full((2, 9), np.nan); bm = np.full(1200, 9, np.uint8); bn = np.full(2, -7, np.int32); bi = np.full(2, -7, np.int32)
        assert g._L.dvs_find_fundamental_cv_batch(g._h, 2, _p(off), _p(p1), _p(p2), THR_F, CONF, 1000, _p(F9), _p(bm), _p(bn), _p(bi)) == 0
        for b, prob in enumerate(order):
            want = (F, mask, nin, its) if prob is long_p else (Fs, masks, nins, itss)
            assert F9[b].tobytes() == want[0].tobytes() and (bm[off[b]:off[b + 1]] == want[1]).all() and (bn[b], bi[b]) == want[2:], b
    g.close()


# ------------------------------------------------------------------ LMedS
@pytest.mark.parametrize("key", LMEDS_KEYS)
def test_lmeds(lmeds_runs, key):
    (p1, p2), out = lmeds_runs[key]
    n = len(p1)
    sel = out["sel"]
    assert sel[1] == LMEDS_ITERS and out["found"] == LMEDS_ITERS
    want = ref.lmeds(out["F"], out["valid"], p1, p2, n)
    best = int(sel[0])
    assert best >= 0 and out["valid"][best] == 1
    assert out["Fbest"].tobytes() == out["F"][best].tobytes()
    if n == 14:
        # the median (sorted index 7) is the best error OUTSIDE the model's own seven sample points: a well-defined score
        print(f"{key}: winner {want['winner']}, median {want['median']:.6g}, gap {want['gap']:.3e}")
        assert want["gap"] > 1e-3
        assert best == want["winner"]
        e, thr2 = want["errors"], float(np.float32(want["thr2"]))
        assert ref.count_float(e, thr2)[1] == 0, "an error within rounding of sigma^2: inconclusive, choose another seed"
        check_mask(out["mask"], e, thr2)
        assert out["mask"].sum() == sel[2] == want["count"] and sel[3] == want["success"]
    else:
        # index n // 2 < 7: EVERY model's median is the error of one of its own sample points, rounding noise around zero, and which model
        # wins is decided by that noise.  What the rule defines: the winner's median and the smallest are both below 1e-6 px^2, sigma is at
        # its floor or next to it, the inliers follow from the WINNER's own median
        assert want["medians"][best] < 1e-6 and want["median"] < 1e-6
        e = ref.epipolar_error(out["F"][best], p1, p2)
        med = float(np.sort(e.astype(np.float32))[n // 2])
        sigma = max(2.5 * 1.4826 * (1 + 5.0 / (n - 7)) * np.sqrt(med), 0.001)
        check_mask(out["mask"], e, float(np.float32(sigma * sigma)))
        assert out["mask"].sum() == sel[2] and sel[3] == int(sel[2] >= 7)


# ------------------------------------------------------------------ PnP: samples and EPnP hypotheses
@pytest.mark.parametrize("key", PNP_KEYS)
def test_epnp_samples_and_hypotheses(pnp_runs, key):
    from dvslam_amd import glue
    (X, uv, K4, behind, R, t), out = pnp_runs[key]
    n = len(X)
    if n < 6:                                                                          # refused inside the batch
        assert (out["samples"] == 0).all() and (out["models"] == 0).all() and (out["counts"] == 0).all()
        assert tuple(out["sel"]) == (-1, 0, 0, 0) and out["nin"] == 0 and out["ok"] == 0 and (out["rvec"] == 0).all() and (out["tvec"] == 0).all()
        assert (out["tail"] == -7).all()
        return
    idx = glue.cv_ransac_subsets_nocheck(n, 5, H)
    assert out["samples"].tolist() == idx.tolist()
    fits, fit_of = 0, [False] * H
    for h in range(H):
        m = out["models"][h]
        Rm = m[6:15].reshape(3, 3)
        assert np.isfinite(m).all(), h
        assert np.abs(Rm - ref.rodrigues_to_R(m[:3])).max() <= 1e-15, h
        assert np.abs(Rm @ Rm.T - np.eye(3)).max() <= 1e-12 and abs(np.linalg.det(Rm) - 1) <= 1e-12, h
        # EPnP fixes the sign on the first point's depth in its control-point solution, BEFORE the rigid fit that gives (R, t): what the pose
        # itself says about that point follows only where the fit reproduces the solution, i.e. where the sample is consistent — its five
        # points come back within 1 px (depths here are 1 .. 3, so the fitted depth is the solution's to a few per cent).  A sample with
        # an outlier or a point moved behind the camera has no rigid solution, and its pose may put the first point behind the camera
        # (the CPU oracle's EPnP does the same: 5 of the 100 samples of n = 257, 17 of planar 257).
        if ref.proj_err_float(Rm, m[3:6], K4, X[idx[h]], uv[idx[h]]).max() < 1.0:
            fits += 1; fit_of[h] = True
            assert (X[idx[h, 0]].astype(np.float64) @ Rm.T + m[3:6])[2] > 0, h
    print(f"{key}: {fits} / {H} hypotheses reproduce their own sample within 1 px")
    assert fits >= 1
    if key.startswith("exact") and "planar" not in key:
        # noise-free and not planar: EPnP recovers the true pose from every sample that holds no point moved behind the camera
        rt = rodrigues(R)
        clean = [h for h in range(H) if not set(idx[h].tolist()) & set(behind.tolist())]
        worst = max(max(np.abs(out["models"][h, :3] - rt).max(), np.abs(out["models"][h, 3:6] - t).max()) for h in clean)
        print(f"{key}: {len(clean)} clean samples, kernel - truth {worst:.3e}")
        assert len(clean) > 0.7 * H and worst <= TRUE_POSE_TOL
        # every clean sample has the true pose, which reprojects it exactly and in front of the camera: the depth check above ran on all of them
        assert fits >= len(clean) and all(fit_of[h] for h in clean)


@pytest.mark.parametrize("Hn", H_VALUES)
def test_epnp_group_packing_does_not_leak(stages, pnp_runs, Hn):
    """k_epnp_hypotheses packs four hypotheses into a workgroup: any H gives the same first models, byte for byte, as H = 100"""
    (X, uv, K4, behind, R, t), full = pnp_runs["n257"]
    out = full if Hn == H else stages.pnp([(X, uv)], K4, H=Hn)[0]
    m = min(Hn, H)
    assert out["samples"][:m].tobytes() == full["samples"][:m].tobytes()
    assert out["models"][:m].tobytes() == full["models"][:m].tobytes()
    assert (out["counts"][:m] == full["counts"][:m]).all()


@pytest.mark.parametrize("Hn", H_VALUES)
def test_f7_block_packing_does_not_leak(stages, fm_runs, Hn):
    """k_f7_hypotheses packs 64 samples into a workgroup"""
    (p1, p2), full = fm_runs["n257"]
    out = full if Hn == H else stages.fm([(p1, p2)], H=Hn)[0]
    m = min(Hn, H)
    assert out["F"][:3 * m].tobytes() == full["F"][:3 * m].tobytes() and (out["valid"][:3 * m] == full["valid"][:3 * m]).all()
    assert (out["counts"][:3 * m] == full["counts"][:3 * m]).all()


# ------------------------------------------------------------------ PnP: score, select, inlier list, refit through the estimator
@pytest.mark.parametrize("key", [k for k in PNP_KEYS if k not in ("ragged1", "ragged2")])
def test_pnp_score_select_inliers_refit(stages, pnp_runs, key):
    (X, uv, K4, behind, R, t), out = pnp_runs[key]
    n = len(X)
    thr2 = float(np.float32(THR_P * THR_P))
    e = np.stack([ref.proj_err_float(m[6:15], m[3:6], K4, X, uv).astype(np.float64) for m in out["models"]])
    check_counts(out["counts"], e, thr2)
    best, it, cnt, more, margin = ref.replay_select_cv(out["counts"], n, 5, CONF, 1, H, H)
    assert margin > 1e-6
    assert tuple(out["sel"]) == (best, it, cnt, more) and more == 0
    assert best >= 0
    sure_in = e[best] < thr2 * (1 - ref.BAND_F); sure_out = e[best] > thr2 * (1 + ref.BAND_F)
    inl = out["inliers"]
    assert (np.diff(inl) > 0).all() and set(np.flatnonzero(sure_in).tolist()) <= set(inl.tolist()) and not set(np.flatnonzero(sure_out).tolist()) & set(inl.tolist())
    assert out["nin"] == out["sel"][2] == len(inl)
    assert (out["tail"] == -7).all()                                                   # nothing written behind the list
    # the refit alone on the same selected model: the same bytes as the estimator, and the initialisation it started from
    alone = stages.refit(X, uv, K4, out["models"][best][:6])
    assert alone["nin"] == out["nin"] and alone["inliers"][:out["nin"]].tolist() == inl.tolist() and (alone["inliers"][out["nin"]:] == -1).all()
    assert alone["ok"] == out["ok"] and alone["rvec"].tobytes() == out["rvec"].tobytes() and alone["tvec"].tobytes() == out["tvec"].tobytes()
    if out["nin"] < 6:                                                                 # n = 6, 7: five inliers that are not planar — no initialisation
        assert out["ok"] == 0 and alone["path"] == 0 and alone["iters"] == 0
        assert out["rvec"].tobytes() == out["models"][best][:3].tobytes() and out["tvec"].tobytes() == out["models"][best][3:6].tobytes()
        return
    assert out["ok"] == 1 and alone["path"] in (1, 2) and 1 <= alone["iters"] <= 20
    Xi = X[inl].astype(np.float64); uvi = uv[inl].astype(np.float64)
    ro, to = ref.refit_optimum(Xi, uvi, K4, alone["init"][:3], alone["init"][3:])
    d = max(np.abs(ro - out["rvec"]).max(), np.abs(to - out["tvec"]).max())
    print(f"{key}: {len(inl)} inliers, path {alone['path']}, {alone['iters']} LM iterations, kernel - optimum {d:.3e}, bound {REFIT_BOUND:.1e}")
    assert d <= REFIT_BOUND
    if key.startswith("exact"):
        assert max(np.abs(out["rvec"] - rodrigues(R)).max(), np.abs(out["tvec"] - t).max()) <= TRUE_POSE_TOL


# ------------------------------------------------------------------ the refit alone
def _true_model(R, t):
    return np.concatenate([rodrigues(R), t])


@pytest.mark.parametrize("n", [63, 64, 65, 257])
def test_refit_dlt_initialisation(stages, n):
    """non-planar inlier sets that end a 64-lane trip, end the next one, start a third: the true pose as the selected model"""
    X, uv, K4, behind, R, t = rs.pnp_scene(600, outliers=0.0)
    keep = np.setdiff1d(np.arange(600), behind)[:n]
    X, uv = X[keep], uv[keep]
    out = stages.refit(X, uv, K4, _true_model(R, t))
    assert out["nin"] == n and out["inliers"][:n].tolist() == list(range(n)) and out["ok"] == 1
    path, r0, t0 = ref.refit_init(X, uv, K4)
    d = max(np.abs(out["init"][:3] - r0).max(), np.abs(out["init"][3:] - t0).max())
    print(f"n = {n}: kernel - reference initialisation {d:.3e}, bound {INIT_BOUND:.1e}, {out['iters']} LM iterations")
    assert out["path"] == 2 == path and d <= INIT_BOUND
    assert 1 <= out["iters"] <= 20


@pytest.mark.parametrize("n", [65, 257])
def test_refit_planar_initialisation(stages, n):
    X, uv, K4, R, t = rs.planar_inlier_set(n)
    out = stages.refit(X, uv, K4, _true_model(R, t))
    assert out["nin"] == n and out["ok"] == 1
    path, r0, t0 = ref.refit_init(X, uv, K4)
    d = max(np.abs(out["init"][:3] - r0).max(), np.abs(out["init"][3:] - t0).max())
    print(f"planar n = {n}: kernel - reference initialisation {d:.3e}, bound {INIT_BOUND:.1e}, {out['iters']} LM iterations")
    assert out["path"] == 1 == path and d <= INIT_BOUND
    assert 1 <= out["iters"] <= 20


@pytest.mark.parametrize("m", [3, 5])
def test_refit_without_initialisation_returns_the_model(stages, m):
    """a model that leaves m < 6 inliers which are not planar: no initialisation, success 0, the model's bytes come back, the list holds them"""
    X, uv, K4, behind, R, t = rs.pnp_scene(600, noise=0.0, outliers=0.0)
    keep = np.setdiff1d(np.arange(600), behind)[:12]
    X, uv = X[keep], uv[keep].copy()
    uv[m:] += np.float32(50.0)
    model = _true_model(R, t)
    out = stages.refit(X, uv, K4, model)
    assert ref.refit_init(X[:m], uv[:m], K4)[0] == 0
    assert out["nin"] == m and out["inliers"][:m].tolist() == list(range(m)) and (out["inliers"][m:] == -1).all()
    assert out["ok"] == 0 and out["path"] == 0 and out["iters"] == 0 and (out["init"] == 0).all()
    assert out["rvec"].tobytes() == model[:3].tobytes() and out["tvec"].tobytes() == model[3:].tobytes()


@pytest.mark.parametrize("m", [4, 5])
def test_refit_planar_with_four_and_five_inliers(stages, m):
    X, uv, K4, R, t = rs.planar_inlier_set(12, noise=0.0)
    uv = uv.copy(); uv[m:] += np.float32(50.0)
    out = stages.refit(X, uv, K4, _true_model(R, t))
    assert ref.refit_init(X[:m], uv[:m], K4)[0] == 1
    assert out["nin"] == m and out["inliers"][:m].tolist() == list(range(m)) and out["path"] == 1 and out["ok"] == 1 and 1 <= out["iters"] <= 20


def test_refit_inlier_comparison_is_in_float(stages):
    """PnPRansacCallback compares a float error with (float)(thr^2).  thr = 1.1: thr^2 = 1.2100000000000002 in double, 1.21000004 as a float.
    A point on the optical axis seen 1.1f px off the principal point (at 0: the offset is the float itself) has the float error
    1.1f * 1.1f = 1.21000004: an inlier by the float comparison, not by a double one.  The next float offset is out either way."""
    K4 = np.array([600.0, 600.0, 0.0, 0.0])
    X = np.array([[0, 0, 1.0], [0, 0, 2.0], [0, 0, 3.0]], np.float32)
    d = np.float32(1.1)
    uv = np.array([[d, 0], [np.nextafter(d, np.float32(2)), 0], [0, 0]], np.float32)
    e = ref.proj_err_float(np.eye(3), np.zeros(3), K4, X, uv)
    thr = np.float32(1.1 * 1.1)
    assert e[0] == thr and float(e[0]) > 1.1 * 1.1 and e[1] > thr and e[2] == 0
    out = stages.refit(X, uv, K4, np.zeros(6), thr=1.1)
    assert out["nin"] == 2 and out["inliers"].tolist() == [0, 2, -1] and out["ok"] == 0 and out["path"] == 0


def test_refit_with_nothing_selected(stages):
    X, uv, K4, behind, R, t = rs.pnp_scene(65)
    out = stages.refit(X, uv, K4, None)
    assert out["nin"] == 0 and out["ok"] == 0 and (out["rvec"] == 0).all() and (out["tvec"] == 0).all() and (out["inliers"] == -1).all()
    assert out["path"] == 0 and out["iters"] == 0 and (out["init"] == 0).all()


@pytest.mark.parametrize("planar", [False, True])
def test_refit_started_at_the_truth_stops_at_once(stages, planar):
    """noise-free: the initialisation is the true pose to the inputs' rounding, and the loop ends after one or two iterations"""
    if planar:
        X, uv, K4, R, t = rs.planar_inlier_set(257, noise=0.0)
    else:
        X, uv, K4, behind, R, t = rs.pnp_scene(600, noise=0.0, outliers=0.0)
        keep = np.setdiff1d(np.arange(600), behind)[:257]
        X, uv = X[keep], uv[keep]
    out = stages.refit(X, uv, K4, _true_model(R, t))
    assert out["ok"] == 1 and out["path"] == (1 if planar else 2) and out["iters"] in (1, 2)
    assert max(np.abs(out["rvec"] - rodrigues(R)).max(), np.abs(out["tvec"] - t).max()) <= TRUE_POSE_TOL


# ------------------------------------------------------------------ ragged batches equal the single calls
def test_ragged_batches_equal_the_single_calls(stages, fm_runs, lmeds_runs, pnp_runs):
    for i, n in enumerate(RAGGED_F):
        assert _same(fm_runs[f"ragged{i}"][1], fm_runs[f"n{n}"][1]), ("fundamental", i)
    for i, n in enumerate(RAGGED_L):
        alone = lmeds_runs[f"n{n}"][1] if n in L_SIZES else stages.fm([rs.lmeds_scene(n)], H=LMEDS_ITERS)[0]
        assert _same(lmeds_runs[f"ragged{i}"][1], alone), ("lmeds", i)
    probs = ragged_pnp()
    for i, n in enumerate(RAGGED_P):
        if n < 6 or i == 3:
            continue                                                                   # (refused problems: test_epnp_samples_and_hypotheses; problem 3 below)
        assert _same(pnp_runs[f"ragged{i}"][1], pnp_runs[f"n{n}"][1]), ("pnp", i)
    alone = stages.pnp([probs[3][:2]], probs[3][2])[0]                                 # the planar 600-point problem of the batch
    assert _same(pnp_runs["ragged3"][1], alone)


def test_hooks_equal_the_product_calls(pnp_runs, lmeds_runs):
    from dvslam_amd import FrontendGlue
    g = FrontendGlue()
    probs = ragged_pnp()
    batch = g.solve_pnp_ransac_cv_batch([p[0] for p in probs], [p[1] for p in probs], probs[0][2], H, THR_P, CONF)
    for i in range(len(probs)):
        out = pnp_runs[f"ragged{i}"][1]
        assert bool(batch[i][0]) == bool(out["ok"]) and batch[i][3].tolist() == out["inliers"].tolist() and batch[i][4] == out["sel"][1], i
        assert batch[i][1].tobytes() == out["rvec"].tobytes() and batch[i][2].tobytes() == out["tvec"].tobytes(), i
    for n in L_SIZES:
        (p1, p2), out = lmeds_runs[f"n{n}"]
        F, mask, nin, its = g.find_fundamental_cv(p1, p2, THR_F, CONF, 1000)
        assert (mask == out["mask"]).all() and nin == out["sel"][2] and its == LMEDS_ITERS
        assert F.tobytes() == (out["Fbest"] if out["sel"][3] else np.zeros(9)).tobytes()
    g.close()
