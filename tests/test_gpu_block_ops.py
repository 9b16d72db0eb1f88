"""csrc/block_ops.h on its own, through the dvs_test_block_ops hook: one workgroup per case, every thread's
results.  Ranks and counts against numpy.cumsum; the reduction against its contract — thread t folds t + s into t for s = NT/2 .. 1 —
restated in numpy and compared as bit patterns, on doubles whose sum depends on the association.  Every case runs its operation twice
through the same scratch with nothing in between, the second reduction on inputs made from the first one's result."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _flag_patterns():
    rng = np.random.default_rng(5)
    one = lambda t: np.eye(256, dtype=np.uint8)[t]
    pats = {"clear": np.zeros(256, np.uint8), "set": np.ones(256, np.uint8), "waves 0 and 2": np.repeat([1, 0, 1, 0], 64).astype(np.uint8),
            "waves 1 and 3": np.repeat([0, 1, 0, 1], 64).astype(np.uint8), "random": (rng.random(256) < 0.5).astype(np.uint8),
            "sparse": (rng.random(256) < 0.03).astype(np.uint8)}
    pats.update({f"only {t}": one(t) for t in (0, 63, 64, 255)})
    return pats


PATTERNS = _flag_patterns()
# (first trip, second trip): every pattern comes first once and second once, always followed by a different one
PAIRS = list(zip(PATTERNS, list(PATTERNS)[1:] + list(PATTERNS)[:1]))


@pytest.mark.parametrize("first,second", PAIRS)
def test_rank_and_count(gpu, hooks, first, second):
    flags = np.stack([PATTERNS[first], PATTERNS[second]])
    out = np.full((2, 256, 3), -1, np.int32)
    assert hooks.dvs_test_block_ops(3, 256, 1, flags.ctypes.data, out.ctypes.data) == 0
    for trip in range(2):
        f = flags[trip].astype(np.int64)
        incl = np.cumsum(f)
        assert (out[trip, :, 0] == incl - f).all(), (first, second, trip, "rank")
        assert (out[trip, :, 1] == incl[-1]).all(), (first, second, trip, "total")
        assert (out[trip, :, 2] == incl[-1]).all(), (first, second, trip, "count")


def _tree(v, fold):
    """the header's association on v[nv][nt]: thread t folds t + s into t, s = nt/2 .. 1"""
    v = v.copy()
    s = v.shape[1] // 2
    while s >= 1:
        v[:, :s] = fold(v[:, :s], v[:, s:2 * s])
        s //= 2
    return v[:, 0]


OPS = {"sum": (0, np.float64, np.add, np.add), "max": (1, np.float64, np.fmax, np.add), "min": (2, np.uint64, np.minimum, np.bitwise_xor)}


def _inputs(dtype, nv, nt, seed):
    rng = np.random.default_rng(seed)
    if dtype == np.uint64:
        return rng.integers(0, 2 ** 64, (nv, nt), dtype=np.uint64, endpoint=False)
    # magnitudes over 1e-9 .. 1e9, both signs: almost every addition rounds, so another order of additions gives other bits.  Rows
    # are drawn again until that is so: each row's sum in thread order differs from its sum by the tree.
    v = np.empty((nv, nt))
    for k in range(nv):
        while True:
            v[k] = rng.standard_normal(nt) * 10.0 ** rng.uniform(-9, 9, nt)
            if np.add.accumulate(v[k])[-1] != _tree(v[k:k + 1], np.add)[0]:
                break
    assert (np.abs(v) < 1e-8).any() and (np.abs(v) > 1e8).any() and (v < 0).any() and (v > 0).any()
    return v


@pytest.mark.parametrize("op", list(OPS))
@pytest.mark.parametrize("nv", [1, 5, 27])
@pytest.mark.parametrize("nt", [256, 512])
def test_tree_reduction(gpu, hooks, nt, nv, op):
    code, dtype, fold, mix = OPS[op]
    v = _inputs(dtype, nv, nt, 1000 * nt + 10 * nv + code)
    out = np.zeros((2, nv, nt), dtype)
    assert hooks.dvs_test_block_ops(code, nt, nv, v.ctypes.data, out.ctypes.data) == 0
    want1 = _tree(v, fold)
    want2 = _tree(mix(v, want1[:, None]), fold)
    for got, want, what in ((out[0], want1, "first"), (out[1], want2, "second, on the same scratch")):
        assert (got.view(np.uint64) == want.view(np.uint64)[:, None]).all(), (nt, nv, op, what)


def test_unknown_shape_is_refused(gpu, hooks):
    buf = np.zeros(2 * 512, np.float64)
    assert hooks.dvs_test_block_ops(0, 128, 1, buf.ctypes.data, buf.ctypes.data) != 0
    assert hooks.dvs_test_block_ops(0, 256, 2, buf.ctypes.data, buf.ctypes.data) != 0
    assert hooks.dvs_test_block_ops(4, 256, 1, buf.ctypes.data, buf.ctypes.data) != 0
