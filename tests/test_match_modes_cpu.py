"""CPU side of the matcher modes (knnMatch / crossCheck / radiusMatch): the cv-typed C++ driver compiles against the stubs, the numpy
reference (match_modes_ref.py) agrees with a slow per-pair statement of the three rules, and — where OpenCV's Python module exists —
with cv2.BFMatcher itself (a dormant pin: it skips on machines without cv2)."""
import os
import subprocess
import numpy as np
import pytest
import match_modes_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "dynamic-visual-slam_amd", "lib")


def test_modes_driver_compiles_against_stubs(tmp_path, hiplib):
    from dvslam_amd import device_count
    exe = os.path.join(str(tmp_path), "bf_matcher_modes")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "tests", "cpp", "stubs"), os.path.join(ROOT, "tests", "cpp", "bf_matcher_modes.cpp"), "-o", exe,
                           "-L" + LIBDIR, "-ldvslam_hip", "-Wl,-rpath," + LIBDIR, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    q = ref.tie_heavy("near", 20, 1); t = ref.tie_heavy("near", 30, 2)
    src = os.path.join(str(tmp_path), "in.bin")
    with open(src, "wb") as f:
        f.write(np.array([len(q), len(t)], np.int32).tobytes() + q.tobytes() + t.tobytes())
    assert subprocess.call([exe, src, os.path.join(str(tmp_path), "out.txt")]) == (0 if device_count() > 0 else 3)


def _sets():
    rng = np.random.default_rng(4)
    yield rng.integers(0, 256, (9, 32), dtype=np.uint8), rng.integers(0, 256, (13, 32), dtype=np.uint8)
    yield ref.tie_heavy("three", 12, 1), ref.tie_heavy("three", 25, 2)
    yield ref.tie_heavy("zeros_ones", 15, 3), ref.tie_heavy("zeros_ones", 8, 4)
    yield ref.tie_heavy("near", 10, 5), ref.tie_heavy("near", 30, 6)
    q = rng.integers(0, 256, (6, 32), dtype=np.uint8); t = q[[3, 3, 1]].copy()
    yield q, t
    yield rng.integers(0, 256, (4, 32), dtype=np.uint8), np.zeros((0, 32), np.uint8)


def _d(a, b):
    return sum(bin(int(x) ^ int(y)).count("1") for x, y in zip(a, b))


def test_reference_matches_per_pair_statement():
    for q, t in _sets():
        d = ref.distances(q, t)
        nq, nt = len(q), len(t)
        assert all(d[i, j] == _d(q[i], t[j]) for i in range(nq) for j in range(nt))
        for k in [1, 2, 3, 5, nt + 2]:
            idx, dist = ref.knn(d, k)
            for i in range(nq):
                # batchDistance's insertion with K slots: insert if d < dist[K-1], shifting while dist[s] > d
                slots = [(ref.INT32_MAX, -1)] * k
                for j in range(nt):
                    x = int(d[i, j])
                    if x < slots[k - 1][0]:
                        s = k - 1
                        while s > 0 and slots[s - 1][0] > x:
                            slots[s] = slots[s - 1]; s -= 1
                        slots[s] = (x, j)
                assert [int(v) for v in idx[i]] == [j for _, j in slots] and [int(v) for v in dist[i]] == [x for x, _ in slots]
        ci, cd = ref.cross(d)
        for i in range(nq):
            if nt == 0:
                assert ci[i] == -1
                continue
            j = min(range(nt), key=lambda jj: (d[i, jj], jj))
            back = min(range(nq), key=lambda ii: (d[ii, j], ii))
            assert (ci[i], cd[i]) == ((j, d[i, j]) if back == i else (-1, ref.INT32_MAX))
        stable = lambda ds: np.argsort(ds, kind="stable")
        for bound in [-1.0, 0.0, 5.5, 100.0, 256.0, float("nan")]:
            offs, idx, dist = ref.radius(d, bound, stable)
            for i in range(nq):
                want = [(int(d[i, j]), j) for j in range(nt) if float(np.float32(d[i, j])) <= bound]
                got = list(zip(dist[offs[i]:offs[i + 1]].tolist(), idx[offs[i]:offs[i + 1]].tolist()))
                assert got == sorted(want)   # with a stable order: (distance, train index)


def test_radius_order_is_std_sort(oracle):
    """the radius reference takes its permutation from the real std::sort (oracle); above 16 equal elements it is not stable"""
    ds = np.array([5, 3, 5, 5, 1] * 10, np.int32)
    p = np.asarray(ref.std_sort_order(oracle)(ds))
    assert sorted(p.tolist()) == list(range(len(ds))) and (np.diff(ds[p]) >= 0).all()
    assert (p != np.argsort(ds, kind="stable")).any()


def test_reference_against_opencv():
    cv2 = pytest.importorskip("cv2")
    for q, t in list(_sets())[:5]:
        d = ref.distances(q, t)
        bf = cv2.BFMatcher(cv2.NORM_HAMMING)
        for k in [1, 2, 3, len(t) + 2]:
            idx, dist = ref.knn(d, k)
            got = bf.knnMatch(q, t, k=k)
            for i, row in enumerate(got):
                assert [m.trainIdx for m in row] == [j for j in idx[i] if j >= 0]
                assert [int(m.distance) for m in row] == [x for x, j in zip(dist[i], idx[i]) if j >= 0]
        for bound in [0.0, 5.5, 100.0, 256.0]:
            offs, idx, dist = ref.radius(d, bound, lambda ds: np.argsort(ds, kind="stable"))
            got = bf.radiusMatch(q, t, maxDistance=bound)
            for i, row in enumerate(got):   # the multiset per query (the permutation of ties is std::sort's, pinned on the GPU side)
                assert sorted((int(m.distance), m.trainIdx) for m in row) == list(zip(dist[offs[i]:offs[i + 1]].tolist(), idx[offs[i]:offs[i + 1]].tolist()))
        ci, cd = ref.cross(d)
        got = cv2.BFMatcher(cv2.NORM_HAMMING, True).match(q, t)
        assert [(m.queryIdx, m.trainIdx, int(m.distance)) for m in got] == [(i, int(ci[i]), int(cd[i])) for i in range(len(q)) if ci[i] >= 0]
