"""csrc/pose_host.h without a device: the tracker's pose step, publishKeyframe's quaternion and the motion mask's relative pose through
their test hooks, bit for bit against tests/tracker_ref.py (rodrigues, pose_step — the loops of _track_ref —, quat_xyzw) and against the
relative pose restated here product by product.  The cases sit where the arithmetic branches: the identity below |rvec| = 1e-15, the two
motion-outlier comparisons at equality and one ulp past it, the clamp of the cosine, and a long chain in which R_ accumulates."""
import ctypes as C
import math
import numpy as np
import pytest
import tracker_ref as tr

dbl, vp = C.c_double, C.c_void_p


@pytest.fixture(scope="module")
def H(hooks):
    hooks.dvs_test_tracker_pose_step.argtypes = [vp, vp, vp, vp, dbl, dbl, vp]; hooks.dvs_test_tracker_pose_step.restype = C.c_int32
    hooks.dvs_test_tracker_relative_pose.argtypes = [vp] * 6; hooks.dvs_test_tracker_relative_pose.restype = None
    return hooks


def _f64(a):
    return np.ascontiguousarray(np.asarray(a, np.float64))


def step(H, R, t, rvec, tvec, max_translation=0.5, max_rotation=0.2):
    """the hook -> (updated, R (3, 3), t (3), cv::Rodrigues(rvec) as the step computes it)"""
    R = _f64(R).reshape(9).copy(); t = _f64(t).copy(); rvec = _f64(rvec); tvec = _f64(tvec); rod = np.zeros(9)
    u = H.dvs_test_tracker_pose_step(R.ctypes.data, t.ctypes.data, rvec.ctypes.data, tvec.ctypes.data, max_translation, max_rotation, rod.ctypes.data)
    return bool(u), R.reshape(3, 3), t, rod.reshape(3, 3)


def check_step(H, R, t, rvec, tvec, max_translation=0.5, max_rotation=0.2):
    """one step through the hook and through the reference: the same verdict, the same bits -> (updated, R, t)"""
    u, Rn, tn, rod = step(H, R, t, rvec, tvec, max_translation, max_rotation)
    wu, wR, wt = tr.pose_step([list(map(float, r)) for r in np.asarray(R)], list(map(float, t)), rvec, tvec, max_translation, max_rotation)
    assert rod.tobytes() == _f64(tr.rodrigues([float(v) for v in rvec])).tobytes()
    assert u == wu and Rn.tobytes() == _f64(wR).tobytes() and tn.tobytes() == _f64(wt).tobytes()
    return u, Rn, tn


R0 = tr.rodrigues([0.3, -0.2, 0.5])
T0 = [0.25, -1.5, 0.75]


@pytest.mark.parametrize("scale", [0.0, 0.999e-15, 1.001e-15])
def test_rotation_vector_zero_and_around_the_identity_threshold(H, scale):
    rvec = [scale * 0.6, 0.0, scale * 0.8]                       # |rvec| = scale to rounding: below the threshold, or just above it
    th = math.sqrt((rvec[0] * rvec[0] + rvec[1] * rvec[1]) + rvec[2] * rvec[2])
    assert (th < 1e-15) == (scale < 1e-15)
    u, Rn, tn = check_step(H, R0, T0, rvec, [0.01, -0.02, 0.03])
    assert u
    if scale < 1e-15:                                            # the identity: R_ is multiplied by exact zeros and ones
        assert Rn.tobytes() == _f64(R0).tobytes()


def test_translation_norm_at_the_limit_and_one_ulp_above(H):
    rvec, tvec = [0.01, -0.02, 0.015], [0.11, -0.07, 0.05]
    _, _, norm, _ = tr.inverse_motion(rvec, tvec)
    assert check_step(H, R0, T0, rvec, tvec, max_translation=norm)[0]                                  # tn > max is false at equality
    assert not check_step(H, R0, T0, rvec, tvec, max_translation=math.nextafter(norm, 0.0))[0]        # one ulp above the limit
    u, Rn, tn, _ = step(H, R0, T0, rvec, tvec, max_translation=math.nextafter(norm, 0.0))
    assert not u and Rn.tobytes() == _f64(R0).tobytes() and tn.tobytes() == _f64(T0).tobytes()           # an outlier leaves the pose alone
    # and the rotation limit the same way
    _, _, _, ca = tr.inverse_motion(rvec, tvec)
    ang = math.acos(ca)
    assert check_step(H, R0, T0, rvec, tvec, max_rotation=ang)[0]
    assert not check_step(H, R0, T0, rvec, tvec, max_rotation=math.nextafter(ang, 0.0))[0]


def test_cosine_outside_minus_one_to_one_is_clamped(H):
    """The cosine handed to acos, before the clamp.  Above 1 it cannot get: every diagonal entry of rodrigues() is fl(c + fl((1 - c) k^2))
    with k^2 <= 1 and 1 - c exact, so none exceeds 1 and the trace stays <= 3 — the sweep below asserts that over the tiny rotations
    where rounding could matter, and that the cosine is exactly 1 there (angle 0: no outlier even under a rotation limit of 0).  Below -1
    it does get: at |rvec| = pi, c = -1 and the trace is -3 + 2 (kx^2 + ky^2 + kz^2), whose rounded sum can fall short of 1.  There the
    clamp decides: acos would give NaN, NaN > max_rotation is false, and a half turn would pass as no outlier."""
    rng = np.random.default_rng(5)
    high = 0.0
    for _ in range(2000):
        rvec = list(rng.normal(0, 1, 3) * 10.0 ** rng.uniform(-9, -7))
        ca = tr.inverse_motion(rvec, [0.0, 0.0, 0.0])[3]
        high = max(high, ca)
        if ca == 1.0:
            assert check_step(H, R0, T0, rvec, [0.001, 0.002, -0.001], max_rotation=0.0)[0]
    assert high == 1.0
    low = None
    for _ in range(20000):
        d = rng.normal(0, 1, 3)
        rvec = list(d * (math.pi / np.linalg.norm(d)))
        if tr.inverse_motion(rvec, [0.0, 0.0, 0.0])[3] < -1.0:
            low = rvec
            break
    assert low is not None
    assert not check_step(H, R0, T0, low, [0.001, 0.002, -0.001], max_rotation=3.0)[0]      # acos(-1) = pi > 3


def test_two_hundred_chained_small_motions(H):
    rng = np.random.default_rng(17)
    R, t = np.eye(3), np.zeros(3)
    updated = 0
    for k in range(200):
        big = k % 23 == 22                                       # now and then a motion outlier, which the chain must step over
        rvec = rng.normal(0, 0.03 if not big else 0.3, 3); tvec = rng.normal(0, 0.05 if not big else 0.6, 3)
        u, R, t = check_step(H, R, t, rvec, tvec)
        updated += u
    assert 150 < updated < 200
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-12 and np.abs(R - np.eye(3)).max() > 0.1   # still a rotation, far from where it began


def quat(H, R):
    a = np.concatenate([_f64(R).reshape(9), np.zeros(3)]); q = np.zeros(4); R9 = np.zeros(9); t3 = np.zeros(3)
    H.dvs_test_tracker_relative_pose(a.ctypes.data, None, a.ctypes.data, R9.ctypes.data, t3.ctypes.data, q.ctypes.data)
    return q


def test_quaternion_of_the_published_pose(H):
    rng = np.random.default_rng(3)
    for rvec in [[0.0, 0.0, 0.0], [0.3, -0.2, 0.5], [2.5, 0.1, -0.2]] + [list(rng.normal(0, 0.5, 3)) for _ in range(50)]:
        R = tr.rodrigues(rvec)
        assert quat(H, R).tobytes() == _f64(tr.quat_xyzw(R)).tobytes()


def relative_pose_ref(a, b, ref):
    """csrc/pose_host.h's relative_pose: (R, t) poses as nested lists; every product a row-by-column sum in index order"""
    (Ra, ta), (Rf, tf) = a, ref
    Rp, tp = [row[:] for row in Ra], ta[:]
    if b is not None:
        Rb, tb = b
        Rrel = [[Rb[0][i] * Ra[0][j] + Rb[1][i] * Ra[1][j] + Rb[2][i] * Ra[2][j] for j in range(3)] for i in range(3)]
        trel = [Rb[0][i] * (ta[0] - tb[0]) + Rb[1][i] * (ta[1] - tb[1]) + Rb[2][i] * (ta[2] - tb[2]) for i in range(3)]
        Rp = [[Ra[i][0] * Rrel[0][j] + Ra[i][1] * Rrel[1][j] + Ra[i][2] * Rrel[2][j] for j in range(3)] for i in range(3)]
        tp = [Ra[i][0] * trel[0] + Ra[i][1] * trel[1] + Ra[i][2] * trel[2] + ta[i] for i in range(3)]
    R = [[Rf[0][i] * Rp[0][j] + Rf[1][i] * Rp[1][j] + Rf[2][i] * Rp[2][j] for j in range(3)] for i in range(3)]
    t = [Rf[0][i] * (tp[0] - tf[0]) + Rf[1][i] * (tp[1] - tf[1]) + Rf[2][i] * (tp[2] - tf[2]) for i in range(3)]
    return R, t


@pytest.mark.parametrize("with_t2", [False, True])
def test_relative_pose_with_and_without_the_frame_before_last(H, with_t2):
    rng = np.random.default_rng(11 + with_t2)
    for _ in range(20):
        poses = [(tr.rodrigues(list(rng.normal(0, 0.4, 3))), list(rng.normal(0, 1, 3))) for _ in range(3)]
        a, b, ref = poses[0], (poses[1] if with_t2 else None), poses[2]
        flat = [None if p is None else np.concatenate([_f64(p[0]).reshape(9), _f64(p[1])]) for p in (a, b, ref)]
        R9 = np.zeros(9); t3 = np.zeros(3)
        H.dvs_test_tracker_relative_pose(flat[0].ctypes.data, None if b is None else flat[1].ctypes.data, flat[2].ctypes.data, R9.ctypes.data, t3.ctypes.data, None)
        wR, wt = relative_pose_ref(a, b, ref)
        assert R9.tobytes() == _f64(wR).reshape(9).tobytes() and t3.tobytes() == _f64(wt).tobytes()
        # and it is what it says: ref^-1 o prediction, the prediction being T(t-1) itself without a frame before it
        if b is None:
            assert np.abs(R9.reshape(3, 3) - _f64(ref[0]).T @ _f64(a[0])).max() < 1e-12
