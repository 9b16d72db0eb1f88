"""The DEVICE forms of the four robust estimators (csrc/ransac_device.h: fm_own_device, fm_cv_device, pnp_own_device, pnp_cv_device — what the
tracker and the relocalisation call on points that already live on the device) against the HOST entry points of the same estimators, byte
for byte, on the same matcher context and arguments.  Both carve one layout (csrc/ransac_layout.h) and run one pass; a disagreement would
otherwise surface as a different pose many stages later in tests/test_gpu_tracker.py.  The device side goes through the hook of
include/dvslam_hip_test_ransac_device.h.

Compared: the mask; n_inliers, success, rvec, tvec of the 64-byte result record; the ascending inlier list up to its count; the select
record.  NOT compared, because the forms' contract calls them unused or unwritten: the record's bytes 8..15 and list entries past the count
(such bytes hold what the scratch block or the buffer held before)."""
import ctypes as C
import numpy as np
import pytest
import ransac_cv_stage_ref as ref
import ransac_scenes as rs

pytestmark = pytest.mark.gpu

THR_F, THR_P, CONF = 2.0, 4.0, 0.99
FM_OWN, FM_CV, PNP_OWN, PNP_CV = 0, 1, 2, 3
FM_ITERS, PNP_ITERS = 64, 16
FIRST_PASS = 96          # iterations whose models fm_cv's first RANSAC pass fits (kFmCvFirstPass)
FULL_ITERS = 200


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


class Forms:
    """one matcher context; every method runs the host entry point and then the device form on it and returns both sides' outputs"""

    def __init__(self, L):
        self.L = L
        self.h = C.c_void_p()
        assert L.dvs_matcher_create(0, C.byref(self.h)) == 0, L.dvs_last_error()
        vp, i32, dbl = C.c_void_p, C.c_int32, C.c_double
        L.dvs_solve_pnp_ransac_cv_batch.argtypes = [vp, i32, vp, vp, vp, vp, i32, dbl, dbl, vp, vp, vp, vp, vp, vp]

    def close(self):
        self.L.dvs_matcher_destroy(self.h)

    def _device(self, form, a, b, n, cap, K4, iters, thr, seed):
        mask = np.full(cap, 7, np.uint8); rec = np.full(64, 7, np.uint8); inl = np.full(cap, -7, np.int32); sel = np.full(4, -7, np.int32)
        K = None if K4 is None else np.ascontiguousarray(K4, np.float64)
        rc = self.L.dvs_test_ransac_device_form(self.h, form, _p(a), _p(b), n, cap, None if K is None else _p(K), iters, thr, CONF, seed, _p(mask), _p(rec),
                                                _p(inl), _p(sel))
        assert rc == 0, self.L.dvs_last_error()
        return dict(mask=mask, nin=int(rec[0:4].view(np.int32)[0]), ok=int(rec[4:8].view(np.int32)[0]), rvec=rec[16:40].copy(), tvec=rec[40:64].copy(),
                    inl=inl, sel=sel)

    def fm(self, form, p1, p2, iters, cap=None, seed=5):
        p1, p2 = _f32(p1), _f32(p2)
        n = len(p1); cap = max(n, 1) if cap is None else cap
        F = np.zeros(9); mask = np.full(n + 1, 9, np.uint8); nin = C.c_int32(-7); its = C.c_int32(-7)
        if form == FM_OWN:
            rc = self.L.dvs_find_fundamental_ransac(self.h, _p(p1), _p(p2), n, THR_F, CONF, iters, seed, _p(F), _p(mask), C.byref(nin))
        else:
            rc = self.L.dvs_find_fundamental_cv(self.h, _p(p1), _p(p2), n, THR_F, CONF, iters, _p(F), _p(mask), C.byref(nin), C.byref(its))
        assert rc == 0, self.L.dvs_last_error()
        assert mask[n] == 9
        dev = self._device(form, p1, p2, n, cap, None, iters, THR_F, seed)
        return dict(mask=mask[:n], nin=nin.value, its=its.value), dev

    def pnp(self, form, X, uv, K4, iters, seed=9):
        X, uv = _f32(X), _f32(uv)
        n = len(X); K = np.ascontiguousarray(K4, np.float64)
        rv = np.full(3, np.nan); tv = np.full(3, np.nan); inl = np.full(n + 1, -7, np.int32); nin = np.full(1, -7, np.int32); ok = np.full(1, -7, np.int32)
        host = {}
        if form == PNP_OWN:
            rc = self.L.dvs_solve_pnp_ransac(self.h, _p(X), _p(uv), n, _p(K), iters, THR_P, CONF, seed, _p(rv), _p(tv), _p(inl), nin.ctypes.data_as(C.POINTER(C.c_int32)),
                                             ok.ctypes.data_as(C.POINTER(C.c_int32)))
            assert rc == 0, self.L.dvs_last_error()
        else:
            off = np.array([0, n], np.int32); its = np.full(1, -7, np.int32)
            rc = self.L.dvs_solve_pnp_ransac_cv_batch(self.h, 1, _p(off), _p(X), _p(uv), _p(K), iters, THR_P, CONF, _p(rv), _p(tv), _p(inl), _p(nin), _p(ok), _p(its))
            assert rc == 0, self.L.dvs_last_error()
            # the select record itself: the entry point's body through the stage hook (include/dvslam_hip_test_ransac_cv.h)
            smp = np.zeros((iters, 5), np.int32); models = np.zeros((iters, 18)); counts = np.zeros(iters, np.int32); sel = np.full(4, -7, np.int32)
            rv2 = np.zeros(3); tv2 = np.zeros(3); inl2 = np.zeros(n + 1, np.int32); nin2 = np.zeros(1, np.int32); ok2 = np.zeros(1, np.int32)
            rc = self.L.dvs_test_pnp_cv_stages(self.h, 1, _p(off), _p(X), _p(uv), _p(K), THR_P, CONF, iters, _p(smp), _p(models), _p(counts), _p(sel), _p(inl2),
                                               _p(nin2), _p(ok2), _p(rv2), _p(tv2))
            assert rc == 0, self.L.dvs_last_error()
            assert int(its[0]) == sel[1] and int(nin[0]) == sel[2]
            host["sel"] = sel
        assert inl[n] == -7
        host.update(nin=int(nin[0]), ok=int(ok[0]), rvec=rv.view(np.uint8).copy(), tvec=tv.view(np.uint8).copy(), inl=inl[:n])
        dev = self._device(form, X, uv, n, max(n, 1), K, iters, THR_P, seed)
        return host, dev


def same_fm(host, dev, n):
    assert np.array_equal(dev["mask"][:n], host["mask"])
    assert int(dev["mask"][:n].sum()) == host["nin"] or host["nin"] == 0    # (LMedS reports its inliers only where the call succeeded)


def same_pnp(host, dev, pose=True):
    assert (dev["nin"], dev["ok"]) == (host["nin"], host["ok"])
    if pose:
        assert np.array_equal(dev["rvec"], host["rvec"]) and np.array_equal(dev["tvec"], host["tvec"])
    k = host["nin"]
    assert np.array_equal(dev["inl"][:k], host["inl"][:k])
    assert np.all(np.diff(dev["inl"][:k]) > 0)


@pytest.fixture(scope="module")
def forms(gpu, hooks):
    f = Forms(hooks)
    yield f
    f.close()


@pytest.fixture(scope="module")
def hard_scene():
    """300 correspondences of which 60 % are outliers: RANSACUpdateNumIters asks for far more than 200 iterations, so the 96-iteration pass
    must leave the loop unfinished (sel[3] = 1) and fm_cv_device must run the full one.  CHECKED HERE, on the CPU, before any test relies on
    it: the samples of the first 96 iterations (dvs_cv_ransac_subsets, host only), their 7-point models and inlier counts by
    tests/ransac_cv_stage_ref.py, the loop replayed over them."""
    sc = rs.two_view(n=300, outlier_frac=0.6, noise=0.5, seed=11)
    return sc["pts1"], sc["pts2"]


def test_hard_scene_asks_for_the_full_pass(hiplib, hard_scene):
    from ransac_stage_ref import epipolar_error
    p1, p2 = hard_scene
    n = len(p1)
    idx = np.zeros((FIRST_PASS, 7), np.int32); found = C.c_int32(0)
    assert hiplib.dvs_cv_ransac_subsets(_p(_f32(p1)), _p(_f32(p2)), n, 7, FIRST_PASS, _p(idx), C.byref(found)) == 0
    assert found.value == FIRST_PASS
    counts = np.zeros(3 * FIRST_PASS, np.int64)
    for h in range(FIRST_PASS):
        models, _, _ = ref.seven_point(p1, p2, idx[h])
        for k, F in enumerate(models):
            strict, band = ref.count_float(epipolar_error(F, p1, p2), THR_F * THR_F)
            counts[3 * h + k] = strict + band                       # the most a float comparison can count: the loop then asks for the FEWEST iterations
    best, it, best_count, unfinished, _ = ref.replay_select_cv(counts, n, 7, CONF, 3, found.value, FULL_ITERS)
    assert (it, unfinished) == (FIRST_PASS, 1) and best_count < 0.6 * n


# ------------------------------------------------------------------ fm_own_device
@pytest.mark.parametrize("n,cap", [(7, 7), (8, 8), (300, 340)])
def test_fm_own_device(forms, n, cap):
    p1, p2 = rs.fm_scene(n) if n > 8 else rs.lmeds_scene(8)         # (8 points without outliers: every sample is all of them)
    p1, p2 = p1[:n], p2[:n]
    host, dev = forms.fm(FM_OWN, p1, p2, FM_ITERS, cap=cap)
    same_fm(host, dev, n)
    if n == 7:
        assert not dev["mask"][:n].any()                                # fewer than 8 correspondences: a mask of zeros
    else:
        assert int(dev["mask"][:n].sum()) == host["nin"]
    if n == 300:
        assert host["nin"] >= 100                                       # a model was selected: the comparison is not one of two empty masks
    assert np.all(dev["mask"][n:] == 0xff)                              # nothing behind the count is written


# ------------------------------------------------------------------ fm_cv_device
@pytest.mark.parametrize("n", [8, 14])
def test_fm_cv_device_lmeds(forms, n):
    p1, p2 = rs.lmeds_scene(n)
    host, dev = forms.fm(FM_CV, p1, p2, 1000)
    same_fm(host, dev, n)
    assert host["nin"] >= 7                                             # the LMedS call succeeded


def test_fm_cv_device_smallest_ransac(forms):
    p1, p2 = rs.fm_scene(15)
    host, dev = forms.fm(FM_CV, p1, p2, 1000)
    same_fm(host, dev, 15)


def test_fm_cv_device_full_pass(forms, hard_scene):
    p1, p2 = hard_scene
    host, dev = forms.fm(FM_CV, p1, p2, FULL_ITERS)
    same_fm(host, dev, len(p1))
    assert host["its"] > FIRST_PASS                                     # the second pass ran on the host side (test_hard_scene_asks_for_the_full_pass)


# ------------------------------------------------------------------ pnp_own_device
@pytest.mark.parametrize("n", [3, 4, 100])
def test_pnp_own_device(forms, n):
    X, uv, K4 = rs.pnp_scene(n)[:3]
    host, dev = forms.pnp(PNP_OWN, X, uv, K4, PNP_ITERS)
    same_pnp(host, dev)
    if n == 3:
        assert (dev["nin"], dev["ok"]) == (0, 0)                        # cv::solvePnPRansac needs 4 points
    if n == 100:
        assert dev["ok"] == 1 and dev["nin"] >= 50


# ------------------------------------------------------------------ pnp_cv_device
@pytest.mark.parametrize("n", [6, 100])
def test_pnp_cv_device(forms, n):
    X, uv, K4 = rs.pnp_scene(n)[:3]
    host, dev = forms.pnp(PNP_CV, X, uv, K4, PNP_ITERS)
    assert np.array_equal(dev["sel"], host["sel"])
    same_pnp(host, dev, pose=host["sel"][0] >= 0)                       # rvec / tvec are meaningful where a model was selected
    if n == 100:
        assert dev["ok"] == 1 and dev["nin"] >= 50


# ------------------------------------------------------------------ one context through all four, twice
def test_one_context_through_all_forms_twice(gpu, hooks, hard_scene):
    """scratch slot 0 and the pinned block are the context's: a layout that grew (the 200-iteration pass after a 16-iteration one) must not
    disturb the call after it"""
    f = Forms(hooks)
    try:
        X, uv, K4 = rs.pnp_scene(100)[:3]
        for _ in range(2):
            host, dev = f.pnp(PNP_OWN, X, uv, K4, PNP_ITERS); same_pnp(host, dev)
            host, dev = f.fm(FM_CV, *hard_scene, FULL_ITERS); same_fm(host, dev, len(hard_scene[0]))
            host, dev = f.pnp(PNP_CV, X, uv, K4, PNP_ITERS); assert np.array_equal(dev["sel"], host["sel"]); same_pnp(host, dev, pose=host["sel"][0] >= 0)
            host, dev = f.fm(FM_OWN, *rs.fm_scene(300), FM_ITERS, cap=340); same_fm(host, dev, 300)
            host, dev = f.fm(FM_CV, *rs.lmeds_scene(14), 1000); same_fm(host, dev, 14)
    finally:
        f.close()
