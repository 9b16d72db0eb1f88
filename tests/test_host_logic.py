"""CPU: the C-ABI library loads, exports every symbol include/dvslam_hip.h declares, refuses to run
without a GPU (no fallback), and its host-side logic (libstdc++ introsort replica, glibc sincosf
restatement, geometry tables) agrees with the oracle / libc."""
import ctypes as C
import os
import re
import numpy as np
import pytest
from dvslam_amd._lib import test_lib as _hooks   # lib/libdvslam_hip_test.so: the dvs_test_* hooks (not in the product library)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exports_every_declared_symbol(hiplib):
    hdr = open(os.path.join(ROOT, "include", "dvslam_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    names = sorted(set(re.findall(r"\b(dvs_[a-z0-9_]+)\s*\(", hdr)))
    assert len(names) >= 30
    missing = [n for n in names if not hasattr(hiplib, n)]
    assert not missing, f"declared in include/dvslam_hip.h but not exported: {missing}"
    # the test hooks are declared in their own header and exported by the -DDVS_TEST_HOOKS build only
    assert not [n for n in names if n.startswith("dvs_test_")]
    thdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dvslam_hip_test.h")).read(), flags=re.S)
    tnames = sorted(set(re.findall(r"\b(dvs_test_[a-z0-9_]+)\s*\(", thdr)))
    assert len(tnames) == 18   # five of them the RANSAC stage hooks (tests/test_gpu_ransac_stages.py), one csrc/block_ops.h's, one csrc/trust_region.h's,
    #                            one csrc/table_compact.h's
    assert not [n for n in tnames if hasattr(hiplib, n)], "the product library must not export test hooks"
    assert not [n for n in tnames if not hasattr(_hooks(), n)]
    # round 5: the extractor's scheduling / introspection hooks and the handles inside a pipeline are declared in the
    # test header too — internal to the product library (hidden visibility: csrc/pipeline.hip composes the step from them), exported by
    # the test library, which also exports the whole product ABI
    hooks = sorted(set(re.findall(r"\b(dvs_(?:orb|matcher|pipeline)_[a-z0-9_]+)\s*\(", thdr)))
    assert len(hooks) == 20 and "dvs_orb_set_after_fast_event" in hooks and "dvs_pipeline_extractor" in hooks
    assert not [n for n in hooks if hasattr(hiplib, n)], "scheduling hooks must stay internal to the product library"
    assert not [n for n in hooks + names if not hasattr(_hooks(), n)]
    assert not set(hooks) & set(names)
    import subprocess
    exported = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "dynamic-visual-slam_amd", "lib", "libdvslam_hip.so")],
                              capture_output=True, text=True, check=True).stdout
    extra = sorted(set(re.findall(r" T (dvs_[a-z0-9_]+)", exported)) - set(names))
    assert not extra, f"exported by the product library but not declared in include/dvslam_hip.h: {extra}"


def test_environment_switches_fail_loudly(hiplib, monkeypatch):
    """the one table of DVS_* switches (csrc/util.hip): a name the library does not read, or a value outside the switch's set, is
    DVS_ERR_ARG at the first handle creation — with or without a GPU — instead of a silent default"""
    import ctypes as C
    from dvslam_amd import _lib
    h = C.c_void_p()

    def create():
        code = hiplib.dvs_matcher_create(0, C.byref(h))
        if code == 0:
            hiplib.dvs_matcher_destroy(h)
        return code, hiplib.dvs_last_error().decode()
    monkeypatch.setenv("DVS_MATCH_MFMA", "0")
    assert create()[0] in (0, -5)                       # a known switch with an allowed value: fine (no device here: -5)
    monkeypatch.setenv("DVS_MATCH_MFMA", "2")
    code, msg = create()
    assert code == -6 and "DVS_MATCH_MFMA=2" in msg and "allowed: 0, 1" in msg
    monkeypatch.setenv("DVS_MATCH_MFMA", "off")
    assert create()[0] == -6
    monkeypatch.delenv("DVS_MATCH_MFMA")
    monkeypatch.setenv("DVS_MTACH_LDS", "0")            # a typo
    code, msg = create()
    assert code == -6 and "unknown environment switch DVS_MTACH_LDS" in msg
    monkeypatch.delenv("DVS_MTACH_LDS")
    monkeypatch.setenv("DVS_OCT_T", "384")
    p = _lib.OrbParams(500, 1.2, 8, 20, 7, (C.c_int32 * 7)(*([0] * 7)), 1)
    assert hiplib.dvs_orb_create(C.byref(p), 0, C.byref(h)) == -6 and "allowed: 0, 256, 512" in hiplib.dvs_last_error().decode()
    monkeypatch.delenv("DVS_OCT_T")
    assert create()[0] in (0, -5)
    monkeypatch.setenv("DVSLAM_HIP_SO_NOTE", "x")       # not a DVS_ name: none of the library's business
    assert create()[0] in (0, -5)


def test_no_gpu_means_error_not_fallback(hiplib):
    from dvslam_amd import device_count, ORBextractor, BFMatcher, DvsError
    if device_count() > 0:
        pytest.skip("a GPU is visible here")
    with pytest.raises(DvsError) as e:
        ORBextractor(500, 1.2, 8, 20, 7)
    assert e.value.code == -5
    with pytest.raises(DvsError):
        BFMatcher()


def _sort_both(hiplib, oracle, count, ulx):
    """(replica, std::sort) permutations; the rank-pairing restatement the kernel runs is checked on the way."""
    count = np.ascontiguousarray(count, np.int32); ulx = np.ascontiguousarray(ulx, np.int32)
    n = len(count)
    a = np.zeros(n, np.int32); b = np.zeros(n, np.int32); c = np.zeros(n, np.int32)
    _hooks().dvs_test_sort_nodes(count.ctypes.data, ulx.ctypes.data, n, a.ctypes.data)
    oracle.lib().orc_std_sort_nodes(count.ctypes.data, ulx.ctypes.data, n, b.ctypes.data)
    _hooks().dvs_test_sort_nodes_ranked(count.ctypes.data, ulx.ctypes.data, n, c.ctypes.data)
    assert (c == b).all(), "rank-pairing restatement differs from std::sort"
    return a, b


def test_introsort_replica_matches_std_sort(hiplib, oracle):
    rng = np.random.default_rng(123)
    cases = []
    for n in [0, 1, 2, 3, 15, 16, 17, 18, 31, 32, 33, 64, 100, 257, 434, 1000, 1500]:
        for kc, kx in [(2, 2), (3, 40), (50, 5), (1000, 1000), (1, 1)]:
            cases.append((rng.integers(2, 2 + kc, n), rng.integers(0, kx, n) * 7))
    n = 700
    cases.append((np.arange(n), np.zeros(n)))                         # sorted
    cases.append((np.arange(n)[::-1], np.zeros(n)))                   # reversed
    cases.append((np.minimum(np.arange(n), n - np.arange(n)), np.arange(n) % 3))   # organ pipe
    # median-of-3 killer (Musser): drives the introsort into its heapsort fallback
    k = n // 2
    killer = np.zeros(n, np.int64)
    for i in range(k):
        killer[i] = i + 1 if i % 2 == 0 else k + i + (k % 2 == 0 and 0 or 0)
    for i in range(k):
        killer[k + i] = 2 * (i + 1)
    cases.append((killer, np.arange(n) % 5))
    for count, ulx in cases:
        a, b = _sort_both(hiplib, oracle, count, ulx)
        assert (a == b).all()


def test_introsort_random_stress(hiplib, oracle):
    rng = np.random.default_rng(77)
    for _ in range(400):
        n = int(rng.integers(0, 1500))
        kc, kx = int(rng.integers(1, 60)), int(rng.integers(1, 30))
        a, b = _sort_both(hiplib, oracle, rng.integers(2, 2 + kc, n), rng.integers(0, kx, n) * 11)
        assert (a == b).all()


def test_introsort_heapsort_fallback_is_exercised(hiplib, oracle):
    # adversarial input built against libstdc++'s median-of-3: forces depth-limit -> heapsort
    n = 1024
    rng = np.random.default_rng(5)
    # many runs of quicksort-killer style sequences with heavy ties
    for _ in range(20):
        base = np.concatenate([np.arange(1, n // 2 + 1, 2), np.arange(n // 2 + 1, n + 1), np.arange(2, n // 2 + 1, 2)])[:n]
        base = np.resize(base, n)
        rng.shuffle(base[: rng.integers(0, 8)])
        a, b = _sort_both(hiplib, oracle, base // rng.integers(1, 4), rng.integers(0, 3, n))
        assert (a == b).all()


def test_sincosf_restatement_sample(hiplib, oracle):
    rng = np.random.default_rng(9)
    xs = np.concatenate([rng.uniform(0, 6.4, 20000), [0.0, 1e-5, 0.785398, 0.7853982, 1.5707964, 3.1415927, 4.712389, 6.2831855]]).astype(np.float32)
    s1, c1, s2, c2 = (C.c_float() for _ in range(4))
    for x in xs:
        _hooks().dvs_test_sincosf(float(x), C.byref(s1), C.byref(c1))
        oracle.lib().orc_sincosf(float(x), C.byref(s2), C.byref(c2))
        assert s1.value == s2.value and c1.value == c2.value, x


@pytest.mark.parametrize("rows,cols,nf,nl", [(720, 1280, 2000, 8), (480, 640, 500, 8), (240, 320, 300, 5), (1080, 1920, 1000, 8)])
def test_geometry_matches_oracle(hiplib, oracle, rows, cols, nf, nl):
    from dvslam_amd._lib import OrbParams
    p = OrbParams(nf, 1.2, nl, 20, 7, (C.c_int32 * 7)(*([0] * 7)), 1)
    w = np.zeros(nl, np.int32); h = np.zeros(nl, np.int32); nc = np.zeros(nl, np.int32); q = np.zeros(nl, np.int32)
    wc = np.zeros(nl, np.int32); hc = np.zeros(nl, np.int32)
    assert _hooks().dvs_test_geometry(C.byref(p), rows, cols, w.ctypes.data, h.ctypes.data, nc.ctypes.data, q.ctypes.data,
                                    wc.ctypes.data, hc.ctypes.data) == 0
    o = oracle.OracleORB(nf, 1.2, nl, 20, 7)
    assert [o.level_size(cols, rows, l) for l in range(nl)] == list(zip(w.tolist(), h.tolist()))
    assert o.tables()[2].tolist() == q.tolist()
    if (rows, cols) == (720, 1280):
        assert nc.sum() == 1987 and (wc[0], hc[0]) == (36, 37)      # 1 987 cells, L0 cells 36x37


def test_geometry_rejects_sizes_the_reference_divides_by_zero_on(hiplib):
    from dvslam_amd._lib import OrbParams
    p = OrbParams(500, 1.2, 8, 20, 7, (C.c_int32 * 7)(*([0] * 7)), 1)
    assert _hooks().dvs_test_geometry(C.byref(p), 120, 160, None, None, None, None, None, None) == -2


def test_pipelined_schedule_refuses_two_output_sets():
    """the match of batch i + 1 reads batch i's last frame and is enqueued in step i + 2: with two output sets step i + 2 would
    overwrite that set with no event to wait for (dvslam_amd/pipeline.py)"""
    from dvslam_amd.pipeline import StreamingPipeline
    with pytest.raises(ValueError):
        StreamingPipeline(4, 480, 640, nsets=2, pipelined=True)
