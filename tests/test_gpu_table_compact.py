"""csrc/table_compact.h's ordered compaction on its own, through the dvs_test_compact_rows hook: the three steps (count per 256-row block,
scan, gather) on a backend handle's stream and block scratch, with an Emit that stores each flagged row's index at its position.
Against numpy.flatnonzero(flags == 1) and its length, at row counts on both sides of one, two and three blocks."""
import ctypes as C
import numpy as np
import pytest
import backend_ref as br

pytestmark = pytest.mark.gpu
SIZES = [0, 1, 255, 256, 257, 512, 513, 769]


def _patterns(n):
    rng = np.random.default_rng(1000 + n)
    pats = {"none": np.zeros(n, np.int32), "all": np.ones(n, np.int32), "every other": (np.arange(n) % 2 == 0).astype(np.int32),
            "half": (rng.random(n) < 0.5).astype(np.int32), "sparse": (rng.random(n) < 0.03).astype(np.int32)}
    if n:
        pats["first only"] = np.zeros(n, np.int32); pats["first only"][0] = 1
        pats["last only"] = np.zeros(n, np.int32); pats["last only"][-1] = 1
        pats["other values"] = rng.permutation(np.array([2, 1, -1, 0], np.int32)[np.arange(n) % 4])     # 2 and -1 are not flagged
    if n >= 513:
        mid = np.zeros(n, np.int32); mid[256:512] = 1
        pats["middle block only"] = mid
        pats["middle block clear"] = 1 - mid
    return pats


@pytest.fixture(scope="module")
def handle(gpu, hooks):
    """a backend handle of the library with the hooks, without a map"""
    from dvslam_amd import backend as B
    B._bind(hooks)
    hooks.dvs_test_compact_rows.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
    h = C.c_void_p()
    assert hooks.dvs_backend_create(C.byref(B.default_params(br.FX, br.FY, br.CX, br.CY, [])), 0, C.byref(h)) == 0
    yield h
    hooks.dvs_backend_destroy(h)


def _run(hooks, h, flags):
    n = len(flags)
    flags = np.ascontiguousarray(flags, np.int32)
    out = np.full(max(n, 1), -7, np.int32)
    total = C.c_int64(-7)
    assert hooks.dvs_test_compact_rows(h, n, flags.ctypes.data, out.ctypes.data, C.byref(total)) == 0
    return out[:n], total.value


def _check(got, flags, what):
    out, total = got
    want = np.flatnonzero(np.asarray(flags) == 1)
    assert total == len(want), (what, total, len(want))
    assert out[:total].tolist() == want.tolist(), what
    assert (out[total:] == -1).all(), (what, "nothing is written behind the total")


@pytest.mark.parametrize("n", SIZES)
def test_flagged_rows_in_order(hooks, handle, n):
    pats = _patterns(n)
    assert n < 513 or {"middle block only", "middle block clear"} <= set(pats)
    assert n < 4 or all((pats["other values"] == v).any() for v in (0, 1, 2, -1))
    for name, flags in pats.items():
        _check(_run(hooks, handle, flags), flags, (n, name))


def test_a_shorter_call_after_a_longer_one_on_the_same_handle(hooks, handle):
    """769 rows leave four blocks' counts and offsets behind; 255 rows use one: a stale count behind the live range would show in the total"""
    long = np.ones(769, np.int32)
    short = (np.arange(255) % 3 == 0).astype(np.int32)
    _check(_run(hooks, handle, long), long, "769")
    _check(_run(hooks, handle, short), short, "255 after 769")
    _check(_run(hooks, handle, long[:0]), long[:0], "0 after 255")
