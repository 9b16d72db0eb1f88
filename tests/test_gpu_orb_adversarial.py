"""GPU parity of the ORB extractor on adversarial content (tests/adversarial_images.py) against the CPU oracle, with the bar of
test_gpu_orb.py: pyramid bytes, blurred bytes on levels with keypoints, candidate lists in order, quad-tree output per level, all 7
keypoint fields as u32 bits and the descriptors.  synth frames keep candidates sparse, scores untied and pixels mid-grey; this
content drives the quad-tree's HBM point path, the fallback of cells whose corners have no strict maximum, tied responses, zero IC
moments and the 0 / 255 extremes of the kernels' packed arithmetic.  Each test asserts from the oracle that its content still
reaches that case, so the coverage cannot decay silently."""
import os
import numpy as np
import pytest
import adversarial_images as ai
from dvslam_amd import synth
from test_gpu_orb import _assert_same_result

pytestmark = pytest.mark.gpu

HD, ODD = (720, 1280), (481, 643)
DENSE = ["iid_noise", "binary_noise", "checker3", "posterised", "square_grid", "lattice0", "saturated"]
_REF = {}


def _ref(oracle, name, shape, nf=1000, ini=20, mn=7, flip=False):
    """oracle result, pyramid, candidates and quad-tree output of (image, config), computed once per module; flip: the image upside
    down (a second, different frame of the same content)"""
    key = (name, shape, nf, ini, mn, flip)
    if key not in _REF:
        img = ai.make(name, *shape)
        if flip:
            img = np.ascontiguousarray(img[::-1])
        o = oracle.OracleORB(nf, 1.2, 8, ini, mn)
        n, kps, desc = o.extract(img)
        r = dict(img=img, res=(n, kps, desc), level=[o.level(l) for l in range(8)], cand=[o.candidates(l) for l in range(8)])
        r["blurred"] = [o.level(l, blurred=True) if len(o.level_keypoints(l)) else None for l in range(8)]
        r["lk"] = []
        for l in range(8):
            lk = o.level_keypoints(l)
            r["lk"].append(np.stack([lk["x"].astype(np.int32) - 16, lk["y"].astype(np.int32) - 16, lk["response"].astype(np.int32)], axis=1))
        _REF[key] = r
    return _REF[key]


def _require(name, shape, ref, ini=20, mn=7):
    """preconditions: what each image is in the suite for, read off the oracle"""
    cand = [len(c) for c in ref["cand"]]
    if name in ("iid_noise", "binary_noise"):
        # over the quad-tree's LDS point capacity (6144 at most) on >= 4 levels at 720p.  481 x 643 has a third of the pixels: there
        # iid noise has 5 934 candidates on level 3 and binary noise 3 535 on level 0, so the bar is 3 levels
        assert sum(c > 6144 for c in cand) >= (4 if shape == HD else 3), f"{name}: not dense enough for the HBM point path {cand}"
    if name in ("binary_noise", "posterised", "square_grid", "lattice0", "saturated"):
        assert max(int(c[:, 2].max()) for c in ref["cand"] if len(c)) == 254, f"{name}: response 254 not reached"
    if name in ("posterised", "square_grid") and (ini, mn) == (20, 7):
        stats = {}
        for l in range(8):
            ai.cell_fast_candidates(ref["level"][l], ini, mn, stats)
        assert stats["tied_cells"] > 0, f"{name}: no cell with corners at iniThFAST but no strict maximum"
    if name == "posterised" and shape == HD and (ini, mn) == (20, 7):
        assert (ref["res"][1]["angle"] == 0).any(), "posterised: no keypoint with angle exactly 0"
    if name.startswith("stripes"):
        assert ref["res"][0] == 0


def _check_stages(g, ref, frame=0, tag=""):
    for l in range(8):
        assert (g.level(l, frame=frame) == ref["level"][l]).all(), f"{tag}pyramid level {l}"
        got = g.candidates(l, frame=frame)
        assert got.shape == ref["cand"][l].shape and (got == ref["cand"][l]).all(), f"{tag}candidates level {l}"
        got = g.level_keypoints(l, frame=frame)
        assert got.shape == ref["lk"][l].shape and (got == ref["lk"][l]).all(), f"{tag}quad-tree level {l}"
        if ref["blurred"][l] is not None:
            assert (g.level(l, blurred=True, frame=frame) == ref["blurred"][l]).all(), f"{tag}blurred level {l}"


def _variant(env, **kw):
    """an extractor created under `env` (dvs_orb_create reads the switches), the environment restored as the variant test does"""
    from dvslam_amd import ORBextractor
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return ORBextractor(**kw)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.mark.parametrize("shape", [HD, ODD], ids=["720p", "481x643"])   # odd width: partial 4-column groups and strips on every level
@pytest.mark.parametrize("name", list(ai.GENERATORS))
def test_stage_parity_on_adversarial_content(gpu, oracle, name, shape):
    """the frontend's configuration (1000, 1.2, 8, 20, 7), stage by stage through the test library and end to end through the
    product library.  The host entry points copy level 0 into the pyramid block (64-byte pitch), so FAST is k_fast_wave and the
    resize k_resize4 here at either width; test_unaligned_device_rows_run_the_generic_fast_kernel covers k_fast_cell and k_resize"""
    from dvslam_amd import ORBextractor
    ref = _ref(oracle, name, shape)
    _require(name, shape, ref)
    g = ORBextractor(1000, 1.2, 8, 20, 7, hooks=True)
    _assert_same_result(*g(ref["img"]), *ref["res"])
    _check_stages(g, ref)
    g.close()
    gp = ORBextractor(1000, 1.2, 8, 20, 7)
    _assert_same_result(*gp(ref["img"]), *ref["res"])
    gp.close()


@pytest.mark.parametrize("nf,ini,mn", [(2000, 20, 7), (1000, 5, 12)], ids=["2000f", "min>ini"])
@pytest.mark.parametrize("name", DENSE)
def test_feature_budget_and_threshold_order(gpu, oracle, name, nf, ini, mn):
    """2000 features (bigger quad-tree quotas) and minThFAST > iniThFAST (the second call finds a subset of nothing) at 720p"""
    from dvslam_amd import ORBextractor
    ref = _ref(oracle, name, HD, nf, ini, mn)
    _require(name, HD, ref, ini, mn)
    g = ORBextractor(nf, 1.2, 8, ini, mn, hooks=True)
    _assert_same_result(*g(ref["img"]), *ref["res"])
    _check_stages(g, ref)
    g.close()


@pytest.mark.parametrize("shape", [HD, ODD], ids=["720p", "481x643"])
@pytest.mark.parametrize("env", [{"DVS_BLUR_MFMA": "1"}, {"DVS_BLUR_MFMA": "2"}, {"DVS_FAST_BYTE_DMA": "0"}, {"DVS_CASCADE": "0"},
                                 {"DVS_CASCADE": "1"}, {"DVS_OCT_T": "256"}, {"DVS_OCT_T": "512"}],
                         ids=lambda e: ",".join(f"{k}={v}" for k, v in e.items()))
def test_opt_in_kernel_variants_on_dense_content(gpu, oracle, env, shape):
    """every kernel switch on the dense images: a batch of three through extract_batch, then each frame alone with its stages"""
    names = ["iid_noise", "binary_noise", "posterised", "square_grid", "saturated", "checker3"]
    refs = [_ref(oracle, nm, shape) for nm in names]
    for nm, r in zip(names, refs):
        _require(nm, shape, r)
    g = _variant(env, nfeatures=1000, scaleFactor=1.2, nlevels=8, iniThFAST=20, minThFAST=7, max_batch=3, hooks=True)
    for b in range(0, len(names), 3):
        nout, kps, desc = g.extract_batch([r["img"] for r in refs[b:b + 3]])
        for i, r in enumerate(refs[b:b + 3]):
            _assert_same_result(int(nout[i]), kps[i, :nout[i]], desc[i, :nout[i]], *r["res"])
            _check_stages(g, r, frame=i, tag=f"{names[b + i]} batch frame {i}: ")
    for nm, r in zip(names, refs):
        _assert_same_result(*g(r["img"]), *r["res"])
        _check_stages(g, r, tag=f"{nm}: ")
    g.close()


def test_mixed_batch_offsets_and_empty_frames(gpu, oracle):
    """one batch of very different frames — flat, iid noise, synth, 2-px checker, a frame with 0 keypoints in the middle, binary
    noise — through extract_batch and extract_batch_device: per-frame offsets and zero-count frames inside a batch"""
    from dvslam_amd import ORBextractor
    from dvslam_amd._lib import DeviceBuffer, KP_DTYPE
    rows, cols = HD
    frames = [np.full(HD, 128, np.uint8), ai.make("iid_noise", rows, cols), synth.make_frame(4, cols=cols, rows=rows),
              ai.make("checker2", rows, cols), ai.make("stripes3y", rows, cols), ai.make("binary_noise", rows, cols)]
    B = len(frames)
    o = oracle.OracleORB(1000, 1.2, 8, 20, 7)
    refs = [o.extract(f) for f in frames]
    assert refs[0][0] == 0 and refs[4][0] == 0 and min(refs[i][0] for i in (1, 2, 3, 5)) > 500
    g = ORBextractor(1000, 1.2, 8, 20, 7, max_batch=B)
    nout, kps, desc = g.extract_batch(frames)
    for i, r in enumerate(refs):
        _assert_same_result(int(nout[i]), kps[i, :nout[i]], desc[i, :nout[i]], *r)
    cap = g.capacity
    d_img = DeviceBuffer(B * rows * cols).upload(np.stack(frames))
    d_k = DeviceBuffer(B * cap * 28); d_d = DeviceBuffer(B * cap * 32); d_n = DeviceBuffer(B * 4)
    g.extract_batch_device(d_img.ptr, B, rows, cols, cols, rows * cols, d_k.ptr, d_d.ptr, cap, d_n.ptr)
    g.synchronize()
    n3 = d_n.download(np.int32, B); k3 = d_k.download(KP_DTYPE, B * cap).reshape(B, cap); d3 = d_d.download(np.uint8, B * cap * 32).reshape(B, cap, 32)
    for i, r in enumerate(refs):
        _assert_same_result(int(n3[i]), k3[i, :n3[i]], d3[i, :n3[i]], *r)
    g.close()


def test_level_sharded_extraction_on_dense_content(gpu, oracle):
    """three ranks (run one after the other on this GPU) extract their pyramid levels of binary and iid noise; the merged blocks
    equal the whole-frame extraction and the oracle"""
    from dvslam_amd import ORBextractor, _lib
    from dvslam_amd import dist as dvdist
    rows, cols = HD
    world, nimg, nf = 3, 2, 1000
    names = ["binary_noise", "iid_noise"]
    refs = [_ref(oracle, nm, HD) for nm in names]
    frames = np.stack([r["img"] for r in refs])
    d_img = _lib.DeviceBuffer(frames.nbytes).upload(frames)
    ref = ORBextractor(nf, 1.2, 8, 20, 7, max_batch=nimg)
    cap = ref.capacity
    d_k = _lib.DeviceBuffer(nimg * cap * 28); d_d = _lib.DeviceBuffer(nimg * cap * 32); d_n = _lib.DeviceBuffer(nimg * 4)
    ref.extract_batch_device(d_img.ptr, nimg, rows, cols, cols, rows * cols, d_k.ptr, d_d.ptr, cap, d_n.ptr); ref.synchronize()
    n0 = d_n.download(np.int32, nimg); k0 = d_k.download(np.uint8, nimg * cap * 28).reshape(nimg, cap, 28)
    de0 = d_d.download(np.uint8, nimg * cap * 32).reshape(nimg, cap, 32)
    px = [int(np.prod(ref.level_size(rows, cols, l))) for l in range(8)]
    masks = dvdist.level_shards(px, world)
    owner = [next(r for r in range(world) if masks[r] >> l & 1) for l in range(8)]
    bb = ref.level_block_bytes(nimg)
    gathered = _lib.DeviceBuffer(world * bb)
    for r in range(world):
        h = ORBextractor(nf, 1.2, 8, 20, 7, max_batch=nimg)
        h.extract_levels_device(d_img.ptr, nimg, rows, cols, cols, rows * cols, masks[r], gathered.ptr + r * bb); h.synchronize()
        h.close()
    d_k2 = _lib.DeviceBuffer(nimg * cap * 28); d_d2 = _lib.DeviceBuffer(nimg * cap * 32); d_n2 = _lib.DeviceBuffer(nimg * 4)
    ref.merge_levels_device(gathered.ptr, world, owner, nimg, d_k2.ptr, d_d2.ptr, cap, d_n2.ptr); ref.synchronize()
    n1 = d_n2.download(np.int32, nimg); k1 = d_k2.download(np.uint8, nimg * cap * 28).reshape(nimg, cap, 28)
    de1 = d_d2.download(np.uint8, nimg * cap * 32).reshape(nimg, cap, 32)
    assert (n1 == n0).all()
    for f, r in enumerate(refs):
        assert (k1[f, :n0[f]] == k0[f, :n0[f]]).all() and (de1[f, :n0[f]] == de0[f, :n0[f]]).all(), f
        _assert_same_result(int(n0[f]), k0[f, :n0[f]].copy().view(_lib.KP_DTYPE).reshape(-1), de0[f, :n0[f]], *r["res"])
    ref.close()


@pytest.mark.parametrize("layout", ["step643", "offset1"])
@pytest.mark.parametrize("name", list(ai.GENERATORS))
def test_unaligned_device_rows_run_the_generic_fast_kernel(gpu, oracle, name, layout):
    """launch_fast (csrc/orb.hip) takes the workgroup-per-cell k_fast_cell — its own segment test, score, NMS and minThFAST fallback —
    only when the caller's frames are not dword aligned, which only extract_batch_device can pass (level 1 is then resized from them
    by k_resize instead of k_resize4).  Two frames (the image and the
    image upside down) from device memory: 481 x 643 at a tight pitch (odd step and frame stride), and 720p from a base pointer one
    byte past an allocation.  Every stage of both frames against the oracle."""
    from dvslam_amd import ORBextractor
    from dvslam_amd._lib import DeviceBuffer, KP_DTYPE
    shape, pad = (ODD, 0) if layout == "step643" else (HD, 1)
    rows, cols = shape
    refs = [_ref(oracle, name, shape), _ref(oracle, name, shape, flip=True)]
    for r in refs:
        _require(name, shape, r)
    frames = np.stack([r["img"] for r in refs])
    assert ((pad | cols | rows * cols) % 4 != 0)                 # what makes launch_fast pick k_fast_cell
    d_img = DeviceBuffer(pad + frames.nbytes + 64).upload(np.concatenate([np.zeros(pad, np.uint8), frames.ravel()]))
    g = ORBextractor(1000, 1.2, 8, 20, 7, max_batch=2, hooks=True)
    cap = g.capacity
    d_k = DeviceBuffer(2 * cap * 28); d_d = DeviceBuffer(2 * cap * 32); d_n = DeviceBuffer(2 * 4)
    g.extract_batch_device(d_img.ptr + pad, 2, rows, cols, cols, rows * cols, d_k.ptr, d_d.ptr, cap, d_n.ptr)
    g.synchronize()
    n = d_n.download(np.int32, 2); k = d_k.download(KP_DTYPE, 2 * cap).reshape(2, cap); d = d_d.download(np.uint8, 2 * cap * 32).reshape(2, cap, 32)
    for f, r in enumerate(refs):
        _assert_same_result(int(n[f]), k[f, :n[f]], d[f, :n[f]], *r["res"])
        _check_stages(g, r, frame=f, tag=f"frame {f}: ")
    g.close()
