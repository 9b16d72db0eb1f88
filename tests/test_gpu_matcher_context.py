"""The matcher handle as the CONTEXT of the host entry points (csrc/matcher.h): its grow-only staging blocks, the pinned in / out block
with its sequence counter (csrc/io_host.h, PinnedIo), both ways a result comes back (export kernel and polled wait up to a size, a
copy command above it) and the handle's life with and without a stream of its own.  The kernels are checked elsewhere; here a call is
compared with a plain numpy statement where one exists (the arg-min), and otherwise with the same call in another setting that must not
matter: a fresh handle, a batch of one.  Every comparison is an equality of bytes.

Sizes: a RANSAC batch leaves through the export kernel while its result region is at most 65536 bytes.  The F region is
[16 + 72 per problem | one mask byte per point]: 8 problems of 8104 points = 8 x 88 + 64832 = 65536, of 8105 points = 65544 (rounded up
to whole dwords).  The PnP region is [64 per problem | 4 per point]: 4 problems of 4080 points = 256 + 65280 = 65536, of 4081 = 65552.
dvs_match_hamming uses the pinned block up to 16384 rows on either side; 3000 x 3000 rows are 216 000 bytes of it, over its 64 KB floor.
"""
import ctypes as C

import numpy as np
import pytest
import ransac_scenes as rs

pytestmark = pytest.mark.gpu

THR_F, THR_P, CONF = 2.0, 4.0, 0.99


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _desc(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def _argmin_ref(q, t):
    """brute-force Hamming arg-min, ties to the lowest train index (np.argmin returns the first minimum); exact: bit counts in float32"""
    A = np.unpackbits(q, axis=1).astype(np.float32); B = np.unpackbits(t, axis=1).astype(np.float32)
    d = (A.sum(1)[:, None] + B.sum(1)[None, :] - 2.0 * (A @ B.T)).astype(np.int32)
    idx = d.argmin(1).astype(np.int32)
    return idx, d[np.arange(len(q)), idx]


def _match(L, h, q, t):
    idx = np.full(len(q), -7, np.int32); dist = np.full(len(q), -7, np.int32)
    assert L.dvs_match_hamming(h, _p(q), len(q), _p(t), len(t), _p(idx), _p(dist)) == 0, L.dvs_last_error()
    return idx, dist


def _matcher(L):
    h = C.c_void_p()
    assert L.dvs_matcher_create(0, C.byref(h)) == 0, L.dvs_last_error()
    return h


# ------------------------------------------------------------------ 1. grow and reuse
def test_match_hamming_grows_and_reuses_its_blocks(gpu, hiplib):
    L = hiplib
    rng = np.random.default_rng(5)
    h = _matcher(L)
    # small; over the pinned floor (both kinds of block regrow); small again in the grown blocks; over 16384 query rows (copy commands)
    for nq, nt in ((64, 64), (3000, 3000), (64, 64), (16385, 64)):
        q, t = _desc(rng, nq), _desc(rng, nt)
        idx, dist = _match(L, h, q, t)
        ridx, rdist = _argmin_ref(q, t)
        assert (idx == ridx).all() and (dist == rdist).all(), (nq, nt)
        f = _matcher(L)
        fidx, fdist = _match(L, f, q, t)
        L.dvs_matcher_destroy(f)
        assert idx.tobytes() == fidx.tobytes() and dist.tobytes() == fdist.tobytes(), (nq, nt)
    L.dvs_matcher_destroy(h)


# ------------------------------------------------------------------ 2. / 3. both sides of the export threshold
def _fm_batch(L, h, problems, seeds, max_iters):
    nprob = len(problems)
    off = np.zeros(nprob + 1, np.int32); off[1:] = np.cumsum([len(p[0]) for p in problems])
    p1 = np.ascontiguousarray(np.concatenate([p[0] for p in problems]), np.float32)
    p2 = np.ascontiguousarray(np.concatenate([p[1] for p in problems]), np.float32)
    sd = np.asarray(seeds, np.uint64)
    F = np.full((nprob, 9), np.nan); mask = np.full(int(off[-1]), 9, np.uint8); nin = np.full(nprob, -7, np.int32)
    L.dvs_find_fundamental_ransac_batch.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_int32,
                                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    assert L.dvs_find_fundamental_ransac_batch(h, nprob, _p(off), _p(p1), _p(p2), THR_F, CONF, max_iters, _p(sd), _p(F), _p(mask), _p(nin)) == 0, \
        L.dvs_last_error()
    return [(F[b].copy(), mask[off[b]:off[b + 1]].copy(), int(nin[b])) for b in range(nprob)]


def _pnp_batch(L, h, problems, K4, seeds, iterations):
    nprob = len(problems)
    off = np.zeros(nprob + 1, np.int32); off[1:] = np.cumsum([len(p[0]) for p in problems])
    X = np.ascontiguousarray(np.concatenate([p[0] for p in problems]), np.float32)
    uv = np.ascontiguousarray(np.concatenate([p[1] for p in problems]), np.float32)
    sd = np.asarray(seeds, np.uint64); K = np.ascontiguousarray(K4, np.float64)
    rv = np.full((nprob, 3), np.nan); tv = np.full((nprob, 3), np.nan); inl = np.full(int(off[-1]), -7, np.int32)
    nin = np.full(nprob, -7, np.int32); ok = np.full(nprob, -7, np.int32)
    L.dvs_solve_pnp_ransac_batch.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_double, C.c_double,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    assert L.dvs_solve_pnp_ransac_batch(h, nprob, _p(off), _p(X), _p(uv), _p(K), iterations, THR_P, CONF, _p(sd), _p(rv), _p(tv), _p(inl), _p(nin),
                                        _p(ok)) == 0, L.dvs_last_error()
    return [(int(ok[b]), rv[b].copy(), tv[b].copy(), int(nin[b]), inl[off[b]:off[b] + max(int(nin[b]), 0)].copy()) for b in range(nprob)]


def _same(a, b):
    return len(a) == len(b) and all((x.tobytes() == y.tobytes()) if isinstance(x, np.ndarray) else x == y for x, y in zip(a, b))


@pytest.fixture(scope="module")
def scenes():
    """eight two-view scenes of 8105 correspondences, made once; a test takes the first n of each"""
    return [rs.two_view(n=8105, outlier_frac=0.3, noise=0.5, seed=20 + b) for b in range(8)]


@pytest.mark.parametrize("n", [8104, 8105])   # result region of 65536 bytes: the last size of the export kernel; 65544: the copy command
def test_fundamental_batch_on_both_sides_of_the_export_threshold(gpu, hiplib, scenes, n):
    L = hiplib
    problems = [(sc["pts1"][:n], sc["pts2"][:n]) for sc in scenes]
    seeds = [101 + 7 * b for b in range(8)]
    assert 8 * 88 + ((8 * n + 3) & ~3) == (65536 if n == 8104 else 65544)
    h = _matcher(L)
    batch = _fm_batch(L, h, problems, seeds, 8)
    assert sum(r[2] for r in batch) > 0                     # the batch found models: the comparison below is not one of zeros
    for b in range(8):
        alone = _fm_batch(L, h, [problems[b]], [seeds[b]], 8)[0]
        assert _same(batch[b], alone), f"problem {b} of the batch differs from the same problem alone"
    L.dvs_matcher_destroy(h)


@pytest.mark.parametrize("n", [4080, 4081])   # 4 x 64 + 4 x 4 x 4080 = 65536; one point more per problem: the copy command
def test_pnp_batch_on_both_sides_of_the_export_threshold(gpu, hiplib, scenes, n):
    L = hiplib
    problems = [(sc["X"][:n], sc["pts2"][:n]) for sc in scenes[:4]]
    seeds = [55 + 3 * b for b in range(4)]
    assert 4 * 64 + 4 * 4 * n == (65536 if n == 4080 else 65552)
    h = _matcher(L)
    batch = _pnp_batch(L, h, problems, scenes[0]["K4"], seeds, 8)
    assert sum(r[3] for r in batch) > 0
    for b in range(4):
        alone = _pnp_batch(L, h, [problems[b]], scenes[0]["K4"], [seeds[b]], 8)[0]
        assert _same(batch[b], alone), f"problem {b} of the batch differs from the same problem alone"
    L.dvs_matcher_destroy(h)


# ------------------------------------------------------------------ 4. one pinned block and one sequence counter for every caller
def test_entry_points_share_the_pinned_block_and_its_counter(gpu, hiplib, scenes):
    from dvslam_amd import FrontendGlue
    from dvslam_amd._lib import KP_DTYPE
    L = hiplib
    rng = np.random.default_rng(9)
    rows, cols, n = 120, 160, 70                            # 70 keypoints: two trips of 64 in k_filter_depth
    kps = np.zeros(n, KP_DTYPE)
    kps["x"] = rng.uniform(0, cols - 1, n).astype(np.float32); kps["y"] = rng.uniform(0, rows - 1, n).astype(np.float32)
    kps["class_id"] = np.arange(n)
    desc = _desc(rng, n)
    depth = rng.integers(0, 4000, (rows, cols)).astype(np.uint16)   # millimetres: some under 0.3 m, some over 3 m
    q, t = _desc(rng, 300), _desc(rng, 257)
    p1, p2 = scenes[0]["pts1"][:600], scenes[0]["pts2"][:600]

    def calls(g):
        """the four calls in order on one handle; every output as bytes"""
        out = []
        for step in ("depth", "match", "fm", "depth"):
            if step == "depth":
                ok, od, oi = g.filter_depth(kps, desc, depth)
                out.append((len(ok), ok.tobytes(), od.tobytes(), oi.tobytes()))
            elif step == "match":
                idx, dist = _match(L, g._h, q, t)
                out.append((idx.tobytes(), dist.tobytes()))
            else:
                F, mask, nin = g.find_fundamental_ransac(p1, p2, threshold=THR_F, confidence=CONF, max_iters=64, seed=3)
                out.append((F.tobytes(), mask.tobytes(), nin))
        return out

    shared = FrontendGlue()
    got = calls(shared)
    shared.close()
    assert 0 < got[0][0] < n and got[2][2] > 0              # the filter dropped some and kept some; the estimator found a model
    assert got[0] == got[3]
    for k, step in enumerate(("depth", "match", "fm", "depth")):
        fresh = FrontendGlue()
        if step == "depth":
            ok, od, oi = fresh.filter_depth(kps, desc, depth)
            ref = (len(ok), ok.tobytes(), od.tobytes(), oi.tobytes())
        elif step == "match":
            idx, dist = _match(L, fresh._h, q, t)
            ref = (idx.tobytes(), dist.tobytes())
        else:
            F, mask, nin = fresh.find_fundamental_ransac(p1, p2, threshold=THR_F, confidence=CONF, max_iters=64, seed=3)
            ref = (F.tobytes(), mask.tobytes(), nin)
        fresh.close()
        assert got[k] == ref, f"call {k} ({step}) on the shared handle differs from a fresh handle"


# ------------------------------------------------------------------ 5. lifecycle
def test_handle_without_a_call(gpu, hiplib):
    h = _matcher(hiplib)
    hiplib.dvs_matcher_destroy(h)


def test_borrowed_own_and_default_stream(gpu, hooks):
    L = hooks
    L.dvs_matcher_use_own_stream.argtypes = [C.c_void_p]
    rng = np.random.default_rng(6)
    q, t = _desc(rng, 130), _desc(rng, 65)
    ridx, rdist = _argmin_ref(q, t)
    s = C.c_void_p()
    assert L.dvs_stream_create(0, 0, C.byref(s)) == 0
    h = C.c_void_p()
    assert L.dvs_matcher_create_on_stream(0, s, C.byref(h)) == 0, L.dvs_last_error()   # borrowed: the handle has no stream of its own yet
    idx, dist = _match(L, h, q, t)
    assert (idx == ridx).all() and (dist == rdist).all()
    assert L.dvs_matcher_use_own_stream(h) == 0, L.dvs_last_error()                    # creates the owned one
    idx, dist = _match(L, h, q, t)
    assert (idx == ridx).all() and (dist == rdist).all()
    assert L.dvs_matcher_set_stream(h, None) == 0, L.dvs_last_error()                  # the default stream; the owned one stays with the handle
    idx, dist = _match(L, h, q, t)
    assert (idx == ridx).all() and (dist == rdist).all()
    L.dvs_matcher_destroy(h)
    assert L.dvs_stream_destroy(s) == 0


# (batch, lanes asked for) -> (lanes, four-stream form): the lane schedule owns a fourth lane's stream, the two-stream forms a match stream
@pytest.mark.parametrize("B,lanes,expect", [(1, 0, (4, False)), (1, 1, (1, False)), (8, 0, (1, True))])
def test_pipeline_created_stepped_once_and_destroyed(gpu, hiplib, B, lanes, expect):
    from dvslam_amd import _lib, synth
    from dvslam_amd.pipeline import StreamingPipeline
    rows, cols = 240, 320
    frames = np.stack([synth.make_frame(i, cols, rows, seed=77) for i in range(B)])
    synth._CANVAS_CACHE.clear()
    d_img = _lib.DeviceBuffer(frames.nbytes).upload(frames)
    pipe = StreamingPipeline(B, rows, cols, 300, lanes=lanes)
    assert (pipe.lanes, pipe.quadtree_async) == expect
    pipe.step(d_img.ptr)
    pipe.flush()
    pipe.synchronize()
    n, _, _ = pipe.outputs(0)
    assert (n > 0).all()
    pipe.close()
