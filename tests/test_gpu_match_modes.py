"""GPU parity of the matcher modes beside match(): knnMatch, crossCheck and radiusMatch (C-ABI, Python mirror and the cv-typed C++
adapter) against the numpy statement in match_modes_ref.py — bit for bit.  Every knn / cross case runs twice: matrix-core kernels
(default) and DVS_MATCH_MFMA=0 (popcount / histogram kernels)."""
import functools
import os
import subprocess
import numpy as np
import pytest
from dvslam_amd import synth
import match_modes_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "dynamic-visual-slam_amd", "lib")
KS = [1, 2, 3, 4, 5, 8, 16, 64]
MODES = ["mfma", "popcount"]


def _matcher(monkeypatch, mode, **kw):
    from dvslam_amd import BFMatcher
    if mode == "popcount":
        monkeypatch.setenv("DVS_MATCH_MFMA", "0")
    else:
        monkeypatch.delenv("DVS_MATCH_MFMA", raising=False)
    return BFMatcher(**kw)


def _planted(nq, nt):
    """test_match_parity's data: random rows plus exact and near duplicates of a few queries in the train set"""
    q = synth.make_descriptors(nq, 100 + nq); t = synth.make_descriptors(nt, 200 + nt)
    if nt > 10 and nq > 3:
        t[7] = q[2]; t[3] = q[2]; t[nt - 1] = q[2]
        t[5] = q[1]; t[5, 0] ^= 1; t[9] = q[1]; t[9, 31] ^= 128
    return q, t


@functools.lru_cache(maxsize=4)
def _planted_ref(nq, nt):
    q, t = _planted(nq, nt)
    return q, t, ref.distances(q, t)


def _check_knn(m, q, t, d, ks=KS):
    for k in ks:
        idx, dist = m.knn_match(q, t, k)
        ei, ed = ref.knn(d, k)
        assert idx.shape == (len(q), k)
        assert (idx == ei).all() and (dist == ed).all(), f"k = {k}"
        if k == 1:
            mi, md = m.match(q, t)
            assert (idx[:, 0] == mi).all() and (dist[:, 0] == md).all(), "knn k = 1 != match()"


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("nq,nt", [(1, 1), (1, 700), (63, 64), (65, 129), (300, 257), (2000, 2000), (2024, 1999), (5000, 4097)])
def test_knn_parity(gpu, monkeypatch, mode, nq, nt):
    q, t, d = _planted_ref(nq, nt)
    _check_knn(_matcher(monkeypatch, mode), q, t, d)


@pytest.mark.parametrize("mode", MODES)
def test_knn_k_above_train_count(gpu, monkeypatch, mode):
    m = _matcher(monkeypatch, mode)
    for nq, nt in [(40, 3), (5, 1), (70, 2)]:
        q, t = _planted(nq, nt)
        _check_knn(m, q, t, ref.distances(q, t), ks=[2, 3, 4, 5, 8])
    idx, dist = m.knn_match(synth.make_descriptors(4, 1), np.zeros((0, 32), np.uint8), 3)   # empty train: all padding
    assert (idx == -1).all() and (dist == ref.INT32_MAX).all()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", ["three", "zeros_ones", "near"])
def test_knn_tie_heavy(gpu, monkeypatch, mode, kind):
    q = ref.tie_heavy(kind, 700, 1); t = ref.tie_heavy(kind, 1500, 2)
    if kind == "three":   # queries from the same 3 rows: distance-0 runs of ~500 train rows must come out in train order
        q = t[np.random.default_rng(3).integers(0, len(t), 700)]
    _check_knn(_matcher(monkeypatch, mode), q, t, ref.distances(q, t))


def _ragged_jobs(P=64, S=300, seed=5, tie=False):
    rng = np.random.default_rng(seed)
    nq = rng.integers(0, S + 1, P).astype(np.int32); nt = rng.integers(0, S + 1, P).astype(np.int32)
    nq[3] = 0; nt[4] = 0; nq[5] = S; nt[5] = S; nt[6] = 1; nt[7] = 3
    if tie:
        Q = np.stack([ref.tie_heavy("near", S, 10 + p) for p in range(P)]); T = np.stack([ref.tie_heavy("near", S, 90 + p) for p in range(P)])
    else:
        Q = np.stack([synth.make_descriptors(S, 30 + p) for p in range(P)]); T = np.stack([synth.make_descriptors(S, 400 + p) for p in range(P)])
        T[:, 10] = Q[:, 2]; T[:, 20] = Q[:, 2]
    return nq, nt, Q, T


def _device_jobs(nq, nt, Q, T, width):
    from dvslam_amd._lib import DeviceBuffer
    P, S = Q.shape[:2]
    b = dict(q=DeviceBuffer(Q.nbytes).upload(Q), t=DeviceBuffer(T.nbytes).upload(T), nq=DeviceBuffer(4 * P).upload(nq),
             nt=DeviceBuffer(4 * P).upload(nt), i=DeviceBuffer(P * S * width * 4), d=DeviceBuffer(P * S * width * 4))
    return b


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("tie", [False, True])
def test_knn_batch_device_ragged(gpu, monkeypatch, mode, tie):
    m = _matcher(monkeypatch, mode)
    nq, nt, Q, T = _ragged_jobs(tie=tie)
    P, S = Q.shape[:2]
    for k in [1, 2, 3, 4, 5, 8]:
        b = _device_jobs(nq, nt, Q, T, k)
        m.knn_match_batch_device(b["q"].ptr, b["nq"].ptr, S, b["t"].ptr, b["nt"].ptr, S, P, k, b["i"].ptr, b["d"].ptr)
        m.synchronize()
        idx = b["i"].download(np.int32, P * S * k).reshape(P, S, k); dist = b["d"].download(np.int32, P * S * k).reshape(P, S, k)
        for p in range(P):
            ei, ed = ref.knn(ref.distances(Q[p, :nq[p]], T[p, :nt[p]]), k)
            assert (idx[p, :nq[p]] == ei).all() and (dist[p, :nq[p]] == ed).all(), (k, p, nq[p], nt[p])
        for x in b.values():
            x.free()


@pytest.mark.parametrize("mode", MODES)
def test_cross_check_host(gpu, monkeypatch, mode):
    m = _matcher(monkeypatch, mode, cross_check=True)
    cases = [_planted(300, 257), _planted(2000, 2000), _planted(65, 129), (ref.tie_heavy("three", 400, 1), ref.tie_heavy("three", 900, 2)),
             (ref.tie_heavy("zeros_ones", 500, 3), ref.tie_heavy("zeros_ones", 300, 4)), (ref.tie_heavy("near", 800, 5), ref.tie_heavy("near", 800, 6))]
    for q, t in cases:
        ei, ed = ref.cross(ref.distances(q, t))
        idx, dist = m.cross_match(q, t)
        assert (idx == ei).all() and (dist == ed).all()
        mi, md = m.match(q, t)                    # the mirror's match() on a cross_check matcher
        assert (mi == ei).all() and (md == ed).all()
        ki, kd = m.knn_match(q, t, 1)
        assert (ki[:, 0] == ei).all() and (kd[:, 0] == ed).all()
    with pytest.raises(ValueError):
        m.knn_match(q, t, 2)


@pytest.mark.parametrize("mode", MODES)
def test_cross_check_lowest_query_rule(gpu, monkeypatch, mode):
    """queries 4 and 9 are the same row and both pick train row 2: the reverse arg-min of row 2 is query 4 (lowest index), so query 9
    has no mutual match — only the tie rule decides it"""
    m = _matcher(monkeypatch, mode, cross_check=True)
    q = synth.make_descriptors(12, 7); t = synth.make_descriptors(6, 8)
    q[9] = q[4]; t[2] = q[4]; t[2, 5] ^= 16
    idx, dist = m.cross_match(q, t)
    ei, ed = ref.cross(ref.distances(q, t))
    assert (idx == ei).all() and (dist == ed).all()
    assert idx[4] == 2 and dist[4] == 1 and idx[9] == -1 and dist[9] == ref.INT32_MAX


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("tie", [False, True])
def test_cross_check_batch_device(gpu, monkeypatch, mode, tie):
    m = _matcher(monkeypatch, mode)
    nq, nt, Q, T = _ragged_jobs(seed=8, tie=tie)
    P, S = Q.shape[:2]
    b = _device_jobs(nq, nt, Q, T, 1)
    m.cross_match_batch_device(b["q"].ptr, b["nq"].ptr, S, b["t"].ptr, b["nt"].ptr, S, P, b["i"].ptr, b["d"].ptr)
    m.synchronize()
    idx = b["i"].download(np.int32, P * S).reshape(P, S); dist = b["d"].download(np.int32, P * S).reshape(P, S)
    for p in range(P):
        ei, ed = ref.cross(ref.distances(Q[p, :nq[p]], T[p, :nt[p]]))
        assert (idx[p, :nq[p]] == ei).all() and (dist[p, :nq[p]] == ed).all(), (p, nq[p], nt[p])


def _check_radius(m, oracle, q, t, bound, d=None):
    d = ref.distances(q, t) if d is None else d
    offs, idx, dist = m.radius_match(q, t, bound)
    eo, ei, ed = ref.radius(d, bound, ref.std_sort_order(oracle))
    assert (offs == eo).all() and (idx == ei).all() and (dist == ed).all(), bound
    return offs


@pytest.mark.parametrize("bound", [-1.0, 0.0, 63.5, 64.0, 100.0, 256.0, float("nan")])
def test_radius_parity(gpu, oracle, bound):
    from dvslam_amd import BFMatcher
    m = BFMatcher()
    q, t = _planted(300, 700)
    t[100:140] = q[5]; t[200:260] = q[6]; t[200:260, 3] ^= 7   # near duplicates: d = 0 runs and d = 3 runs
    offs = _check_radius(m, oracle, q, t, bound)
    if bound != bound or bound < 0:
        assert offs[-1] == 0


@pytest.mark.parametrize("kind", ["three", "zeros_ones", "near"])
def test_radius_long_tied_lists(gpu, oracle, kind):
    """lists far longer than 16 with many equal distances: std::sort's (unstable) permutation is part of the result"""
    from dvslam_amd import BFMatcher
    m = BFMatcher(cross_check=True)   # radiusMatch ignores crossCheck
    q = ref.tie_heavy(kind, 60, 11); t = ref.tie_heavy(kind, 1200, 12)
    d = ref.distances(q, t)
    for bound in [0.0, 16.0, 100.0, 200.5, 256.0]:
        offs = _check_radius(m, oracle, q, t, bound, d)
    assert np.diff(offs).max() > 300


def test_radius_cap_below_total(gpu, oracle):
    from dvslam_amd import BFMatcher
    m = BFMatcher()
    q = ref.tie_heavy("near", 50, 22); t = ref.tie_heavy("near", 400, 22)   # same seed: near duplicates of the same 5 rows
    eo, ei, ed = ref.radius(ref.distances(q, t), 20.0, ref.std_sort_order(oracle))
    n = int(eo[-1])
    assert n > 100
    offs, idx, dist = m.radius_match(q, t, 20.0, cap=n // 3)
    assert (offs == eo).all() and len(idx) == n // 3
    assert (idx == ei[:n // 3]).all() and (dist == ed[:n // 3]).all()
    offs, idx, dist = m.radius_match(q, np.zeros((0, 32), np.uint8), 20.0)
    assert len(idx) == 0 and (offs == 0).all()


def test_k_zero_is_an_argument_error(gpu):
    from dvslam_amd import BFMatcher, DvsError
    m = BFMatcher()
    q = synth.make_descriptors(10, 1)
    with pytest.raises(DvsError) as e:
        m.knn_match(q, q, 0)
    assert e.value.code == -6
    nq, nt, Q, T = _ragged_jobs(P=8, S=32)
    b = _device_jobs(nq, nt, Q, T, 1)
    with pytest.raises(DvsError) as e:
        m.knn_match_batch_device(b["q"].ptr, b["nq"].ptr, 32, b["t"].ptr, b["nt"].ptr, 32, 8, 0, b["i"].ptr, b["d"].ptr)
    assert e.value.code == -6


def _parse(path):
    out, cur, throws = {}, None, None
    for line in open(path):
        f = line.split()
        if f[0] == "BEGIN":
            cur = out.setdefault(f[1], [])
        elif f[0] == "R":
            cur.append([])
        elif f[0] == "THROWS":
            throws = [int(x) for x in f[1:]]
        else:
            cur[-1].append((int(f[0]), int(f[1]), int(f[2]), float(f[3])))
    return out, throws


@pytest.mark.parametrize("kind", ["planted", "near"])
def test_cpp_adapter_modes(gpu, hiplib, oracle, tmp_path, kind):
    """tests/cpp/bf_matcher_modes.cpp: the cv-typed knnMatch / radiusMatch / crossCheck match() of dvslam::HammingBFMatcher"""
    exe = os.path.join(str(tmp_path), "bf_matcher_modes")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "tests", "cpp", "stubs"), os.path.join(ROOT, "tests", "cpp", "bf_matcher_modes.cpp"), "-o", exe,
                           "-L" + LIBDIR, "-ldvslam_hip", "-Wl,-rpath," + LIBDIR, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    if kind == "planted":
        q, t = _planted(300, 257)
    else:
        q = ref.tie_heavy("near", 120, 31); t = ref.tie_heavy("near", 90, 32)
    src = os.path.join(str(tmp_path), "in.bin"); dst = os.path.join(str(tmp_path), "out.txt")
    with open(src, "wb") as f:
        f.write(np.array([len(q), len(t)], np.int32).tobytes() + q.tobytes() + t.tobytes())
    r = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    got, throws = _parse(dst)
    assert throws == [1, 1, 1]
    d = ref.distances(q, t)
    nq, nt = d.shape

    def lists_from_knn(idx, dist, compact):
        rows = [[(i, int(j), 0, float(x)) for j, x in zip(idx[i], dist[i]) if j >= 0] for i in range(nq)]
        return [r for r in rows if r] if compact else rows

    for k in [1, 2, 3, 5, nt + 3]:
        assert got[f"knn{k}"] == lists_from_knn(*ref.knn(d, k), False), k
    assert got["knn2c"] == lists_from_knn(*ref.knn(d, 2), True)
    order = ref.std_sort_order(oracle)
    for bound, name in [(-1.0, "-1"), (0.0, "0"), (63.5, "63"), (100.0, "100"), (256.0, "256"), (float("nan"), "-7")]:
        offs, idx, dist = ref.radius(d, bound, order)
        rows = [[(i, int(idx[p]), 0, float(dist[p])) for p in range(offs[i], offs[i + 1])] for i in range(nq)]
        assert got["radius" + name] == rows, bound
        assert got["radiusc" + name] == [r for r in rows if r], bound
    offs, idx, dist = ref.radius(d, 100.0, order)
    assert got["crossradius100"] == [[(i, int(idx[p]), 0, float(dist[p])) for p in range(offs[i], offs[i + 1])] for i in range(nq)]
    mi, md = ref.knn(d, 1)
    assert got["match"] == [[(i, int(mi[i, 0]), 0, float(md[i, 0])) for i in range(nq)]]
    ci, cd = ref.cross(d)
    assert got["cross"] == [[(i, int(ci[i]), 0, float(cd[i])) for i in range(nq) if ci[i] >= 0]]
    assert got["crossknn"] == lists_from_knn(ci[:, None], cd[:, None], False)
    assert got["crossknnc"] == lists_from_knn(ci[:, None], cd[:, None], True)
    assert len(got["crossknnc"]) < nq   # some queries have no mutual pair: compaction is exercised
