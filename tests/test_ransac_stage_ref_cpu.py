"""The float64 stage references of tests/ransac_stage_ref.py, checked on the CPU before the kernels are held to them
(tests/test_gpu_ransac_stages.py): against the CPU oracle where it states the same thing, against ground truth and hand-worked
answers otherwise."""
import math
import numpy as np
import ransac_scenes as rs
import ransac_stage_ref as ref


def test_sample_equals_the_oracle_sampler(oracle):
    assert ref.splitmix64(0) == 0xE220A8397B1DCDAF                                    # the published first output of SplitMix64 seeded with 0
    for seed, n, k in ((0, 8, 8), (11, 9, 8), (5, 4, 3), (5, 600, 3), (2 ** 64 - 1, 257, 8), (1 << 63, 600, 8)):
        for h in (0, 1, 63, 64, 199, 999):
            want = oracle.sample_distinct(seed, h, n, k).tolist()
            assert ref.sample(seed, h, n, k) == want, (seed, h, n, k)
            assert len(set(want)) == k


def test_eight_point_recovers_the_true_geometry():
    sc = rs.two_view(n=40, outlier_frac=0.0, noise=0.0, seed=2)
    F, ratio = ref.eight_point(sc["pts1"], sc["pts2"])                                # all 40: least squares
    assert abs(np.linalg.norm(F) - 1) < 1e-12 and abs(np.linalg.det(F)) < 1e-12
    assert rs.sampson_truth_error(F, sc) < 1e-3                                       # float32 pixel coordinates
    rng = np.random.Generator(np.random.PCG64(1))
    for _ in range(20):                                                               # minimal samples: unit norm, singular
        idx = rng.choice(40, 8, replace=False)
        F, ratio = ref.eight_point(sc["pts1"][idx], sc["pts2"][idx])
        assert F is not None and 0 < ratio < 1 and abs(np.linalg.norm(F) - 1) < 1e-12 and abs(np.linalg.det(F)) < 1e-12
    p = np.full((8, 2), 7.0, np.float32)
    assert ref.eight_point(p, p) == (None, 0.0)
    line = np.stack([np.arange(8.0), 2 * np.arange(8.0) + 1], 1)                      # collinear: a null space of more than one dimension
    assert ref.eight_point(line, line + 3)[0] is None


def test_epipolar_error_is_the_point_to_line_distance():
    F = np.array([[0, 0, 0], [0, 0, -1.0], [0, 1.0, 0]])                              # pure x-translation: the epipolar line of (x, y) is the row y
    p1 = np.array([[10.0, 20.0], [5.0, 5.0]]); p2 = np.array([[300.0, 23.0], [1.0, 5.0]])
    assert np.allclose(ref.epipolar_error(F, p1, p2), [9.0, 0.0], atol=1e-12)
    e = ref.reprojection_error2(np.eye(3), [0, 0, 0], [600, 600, 320, 240], np.array([[0.1, 0, 2.0], [0, 0, -1.0], [0, 0, 0]]),
                                np.array([[350.0, 244.0], [320.0, 240.0], [320.0, 240.0]]))
    assert abs(e[0] - 16.0) < 1e-9 and np.isinf(e[1]) and np.isinf(e[2])             # behind the camera / at it: never an inlier


def test_replay_select_on_hand_made_counts():
    for case in ref.SELECT_CASES:
        best, it, cnt, margin = ref.replay_select(case["counts"], ref.SELECT_N, case["model_points"], ref.SELECT_CONFIDENCE, case["group"])
        assert (best, it, cnt) == case["expect"], case["name"]
        assert margin > 1e-6, case["name"]                                            # rint() cannot hang on the last bit of log()
    assert ref.update_num_iters(0.99, 0.1, 3, 100)[0] == 4 and ref.update_num_iters(0.99, 0.2, 8, 1000)[0] == 25
    assert ref.update_num_iters(0.99, 0.0, 8, 1000)[0] == 0 and ref.update_num_iters(0.99, 1.0, 8, 1000)[0] == 1000


def _exact_triangle(rng, planar):
    R = rs.rot(rng.normal(size=3), rng.uniform(0, 0.6)); t = rng.normal(size=3) * 0.3
    P = np.stack([rng.uniform(-1, 1, 3), rng.uniform(-1, 1, 3), np.full(3, 1.5) if planar else rng.uniform(1, 3, 3)], 1)
    Q = P @ R.T + t
    s = np.linalg.norm(Q, axis=1)
    return P, Q / s[:, None], s


def test_p3p_roots_contain_the_true_pose():
    rng = np.random.Generator(np.random.PCG64(5))
    seen = 0
    for planar in (False, True):
        for _ in range(150):
            P, j, s = _exact_triangle(rng, planar)
            sols, sep = ref.p3p_roots(P, j)
            assert 0 <= len(sols) <= 4 and all(b[0] > a[0] for a, b in zip(sols, sols[1:]))
            if sep < 1e-4:
                continue
            seen += 1
            err = min(abs(v - s[2] / s[0]) + abs(u - s[1] / s[0]) for v, u in sols)
            assert err < 1e-8 / sep, (err, sep)                                       # root error of a polynomial: rounding over root separation
    assert seen > 250


def test_rodrigues_round_trips():
    rng = np.random.Generator(np.random.PCG64(7))
    for _ in range(100):
        a = rng.normal(size=3); a /= np.linalg.norm(a)
        for th in (1e-9, 1e-3, 1.0, 3.0, math.pi - 1e-7):
            w = ref.rodrigues(rs.rot(a, th))
            assert np.abs(rs.rodrigues_to_R(w) - rs.rot(a, th)).max() < 1e-12, th
            assert abs(np.linalg.norm(w) - th) < 1e-9
    for a in ([0, 1, -1], [1, 0, 0], [-1, 2, 0]):
        w = ref.rodrigues(rs.rot(a, math.pi))
        assert np.abs(rs.rodrigues_to_R(w) - rs.rot(a, math.pi)).max() < 1e-12
    assert np.abs(ref.rodrigues(np.eye(3))).max() == 0


def test_product_rotation_to_rodrigues_on_the_host(hooks):
    """the conversion that ends k_pnp_refine, compiled for the host (dvs_test_rotation_to_rodrigues): rodrigues_to_R(w) gives R back within
    1e-9 at the angles where such a conversion goes wrong — 0, next to 0, next to pi, pi — for axes with zero components and mixed
    signs.  (Until this test the theta = pi branch took both signs from R01 and R02: (0, 1, -1) / sqrt 2 came back as (0, 2.22, 2.22).)"""
    axes = [[1, 0, 0], [0, 1, 0], [0, 0, -1], [0, 1, -1], [0, -1, 1], [1, -1, 0], [-1, 0, 1], [1, 1, 1], [1, -2, 3], [-3, 2, -1], [-1, -1, 0.001],
            [0.001, 1, -1]]
    for a in axes:
        for th in (0.0, 1e-9, 1.0, math.pi - 1e-7, math.pi):
            R = np.ascontiguousarray(rs.rot(a, th))
            w = np.zeros(3)
            hooks.dvs_test_rotation_to_rodrigues(R.ctypes.data, w.ctypes.data)
            assert np.abs(rs.rodrigues_to_R(w) - R).max() < 1e-9, (a, th, w)
            assert np.linalg.norm(w) <= math.pi + 1e-12
            assert np.abs(w - ref.rodrigues(R)).max() < 1e-9 or th >= math.pi - 1e-12, (a, th, w)   # at pi itself, w and -w are one rotation
