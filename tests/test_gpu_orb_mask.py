"""GPU parity of the masked ORB extraction (dvs_orb_extract*_masked, INTEGRATION.md §B1 "Keep masks") against orb_mask_ref.py — the
oracle's own stages with the candidate lists filtered by the keep rule — bit for bit: all 7 keypoint fields as u32 patterns and the
descriptors.  Masks: YOLO-like boxes, random speckle, a small kept window that empties the upper levels, all-zero, all-ones (= the
unmasked call), values 1..255 (= 255) and a padded mask_step.  Routes: the host entry points, the unaligned-row FAST kernel
(k_fast_cell), the serial schedule (overlap off) and batch-device calls with per-frame and shared masks at 8 and 64 frames."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest
import orb_mask_ref as mref
from dvslam_amd import synth
from dvslam_amd._lib import DeviceBuffer, KP_DTYPE
from test_gpu_orb import _assert_same_result
from test_orb_mask_cpu import boxes_mask

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "dynamic-visual-slam_amd", "lib")
ROWS, COLS = 720, 1280
MASKS = ["boxes", "speckle", "window", "zeros", "ones", "values"]
_REF = {}


def make_mask(kind, rows=ROWS, cols=COLS, seed=0, at=None):
    rng = np.random.default_rng(100 + seed)
    if kind == "boxes":
        return boxes_mask(rows, cols, seed=seed)
    if kind == "speckle":
        return (rng.random((rows, cols)) < 0.6).astype(np.uint8) * 255
    if kind == "window":   # 7 x 7 kept pixels (around `at`, a level-0 keypoint): most coarse levels have no candidate inside
        m = np.zeros((rows, cols), np.uint8)
        x, y = at if at is not None else (cols // 3 + 11 * seed, rows // 3 + 7 * seed)
        m[y - 3:y + 4, x - 3:x + 4] = 1
        return m
    if kind == "zeros":
        return np.zeros((rows, cols), np.uint8)
    if kind == "ones":
        return np.ones((rows, cols), np.uint8)
    if kind == "values":   # every nonzero value keeps: the same result as the same mask at 255
        m = (rng.random((rows, cols)) < 0.7).astype(np.uint8)
        return (m * rng.integers(1, 256, (rows, cols))).astype(np.uint8)
    raise ValueError(kind)


def _ref(oracle, t, nf=2000):
    key = (t, nf)
    if key not in _REF:
        _REF[key] = mref.MaskedRef(oracle, synth.make_frame(t, cols=COLS, rows=ROWS), nf)
    return _REF[key]


def _extractor(nf=2000, max_batch=1, hooks=False):
    from dvslam_amd import ORBextractor
    return ORBextractor(nf, 1.2, 8, 20, 7, max_batch=max_batch, hooks=hooks)


@pytest.mark.parametrize("kind", MASKS)
def test_host_masked_matches_reference(gpu, oracle, kind):
    r = _ref(oracle, 0)
    k0 = r.result[1][r.result[1]["octave"] == 0][50]
    mask = make_mask(kind, at=(int(k0["x"]), int(k0["y"])))
    want = r.extract(mask)
    g = _extractor()
    got = g.extract_masked(r.img, mask)
    _assert_same_result(*got, *want)
    if kind == "ones":
        _assert_same_result(*got, *g(r.img))
        _assert_same_result(*got, *r.result)
    if kind == "zeros":
        assert got[0] == 0
    if kind == "values":
        _assert_same_result(*got, *g.extract_masked(r.img, (mask != 0).astype(np.uint8) * 255))
    if kind == "window":
        per_level = np.bincount(want[1]["octave"], minlength=8)
        assert per_level[0] > 0 and (per_level == 0).sum() >= 2, per_level
    if kind in ("boxes", "speckle"):
        assert 0 < got[0] and not np.array_equal(got[1], r.result[1])
    xi = np.floor(got[1]["x"]).astype(np.int64); yi = np.floor(got[1]["y"]).astype(np.int64)
    assert (mask[yi, xi] != 0).all()


def test_padded_mask_step_and_bad_step(gpu, oracle):
    r = _ref(oracle, 1)
    mask = make_mask("boxes", seed=1)
    padded = np.zeros((ROWS, COLS + 24), np.uint8)
    padded[:, :COLS] = mask
    padded[:, COLS:] = 255   # bytes past cols are never read as keep flags
    g = _extractor()
    _assert_same_result(*g.extract_masked(r.img, padded[:, :COLS]), *r.extract(mask))
    # mask_step < cols is an argument error
    from dvslam_amd._lib import ptr
    kps = np.zeros(g.capacity, KP_DTYPE); desc = np.zeros((g.capacity, 32), np.uint8); n = C.c_int32()
    st = g._L.dvs_orb_extract_masked(g._h, ptr(r.img), ROWS, COLS, COLS, ptr(mask), COLS - 1, ptr(kps), ptr(desc), g.capacity, C.byref(n))
    assert st != 0
    # a NULL mask is the unmasked entry point
    st = g._L.dvs_orb_extract_masked(g._h, ptr(r.img), ROWS, COLS, COLS, None, 0, ptr(kps), ptr(desc), g.capacity, C.byref(n))
    assert st == 0
    _assert_same_result(n.value, kps[:n.value], desc[:n.value], *r.result)


def test_filtered_candidates_and_honour_switch(gpu, oracle):
    r = _ref(oracle, 2)
    mask = make_mask("boxes", seed=2)
    g = _extractor(hooks=True)
    got = g.extract_masked(r.img, mask)
    for l, want in enumerate(r.filtered_candidates(mask)):
        c = g.candidates(l)
        assert c.shape == want.shape and (c == want).all(), f"candidates level {l}"
    _assert_same_result(*got, *r.extract(mask))
    # operator() ignores the mask unless honour_mask is on
    p = _extractor()
    _assert_same_result(*p(r.img, mask), *r.result)
    p.honour_mask(True)
    _assert_same_result(*p(r.img, mask), *got)
    _assert_same_result(*p(r.img, None), *r.result)
    p.honour_mask(False)
    _assert_same_result(*p(r.img, mask), *r.result)
    # host batch form
    nout, k, d = p.extract_batch([r.img, r.img], masks=[mask, np.ones_like(mask)])
    _assert_same_result(nout[0], k[0, :nout[0]], d[0, :nout[0]], *got)
    _assert_same_result(nout[1], k[1, :nout[1]], d[1, :nout[1]], *r.result)


@pytest.mark.parametrize("overlap", [1, 0])
def test_overlap_schedules(gpu, oracle, overlap):
    """overlap on (the in-step level chain beside per-level FAST launches at 16 frames) and off (every stage on one stream)"""
    B = 16
    frames = [_ref(oracle, t % 4) for t in range(B)]
    masks = [make_mask(MASKS[t % len(MASKS)], seed=t) for t in range(B)]
    g = _extractor(max_batch=B, hooks=True)
    g.set_overlap(overlap)
    _run_device(g, frames, masks, shared=False)


def test_unaligned_row_route(gpu, oracle):
    """rows that are not dword aligned (step = cols + 1) take k_fast_cell; the filter follows it as well"""
    B = 3
    frames = [_ref(oracle, t) for t in range(B)]
    masks = [make_mask(k, seed=t) for t, k in enumerate(["boxes", "speckle", "window"])]
    _run_device(_extractor(max_batch=B), frames, masks, shared=False, step=COLS + 1)


@pytest.mark.parametrize("B", [8, 64])
@pytest.mark.parametrize("shared", [False, True])
def test_batch_device(gpu, oracle, B, shared):
    frames = [_ref(oracle, t % 8) for t in range(B)]
    masks = [make_mask("boxes", seed=0)] if shared else [make_mask(MASKS[t % 5], seed=t) for t in range(B)]
    _run_device(_extractor(max_batch=B), frames, masks, shared=shared)


def _run_device(g, frames, masks, shared, step=COLS):
    B = len(frames)
    imgs = np.zeros((B, ROWS, step), np.uint8)
    for i, r in enumerate(frames):
        imgs[i, :, :COLS] = r.img
    mstep = COLS + 8
    mk = np.zeros((len(masks), ROWS, mstep), np.uint8)
    for i, m in enumerate(masks):
        mk[i, :, :COLS] = m
        mk[i, :, COLS:] = 255   # padding: never read
    d_img = DeviceBuffer(imgs.nbytes + 64).upload(imgs)
    d_mask = DeviceBuffer(mk.nbytes).upload(mk)
    cap = g.capacity
    d_k = DeviceBuffer(B * cap * KP_DTYPE.itemsize); d_d = DeviceBuffer(B * cap * 32); d_n = DeviceBuffer(4 * B)
    g.extract_batch_device(d_img.ptr, B, ROWS, COLS, step, ROWS * step, d_k.ptr, d_d.ptr, cap, d_n.ptr,
                           d_masks=d_mask.ptr, mask_step=mstep, mask_frame_stride=0 if shared else ROWS * mstep)
    g.synchronize()
    n = d_n.download(np.int32, B)
    k = d_k.download(KP_DTYPE, B * cap).reshape(B, cap)
    d = d_d.download(np.uint8, B * cap * 32).reshape(B, cap, 32)
    want = {}
    for f in range(B):
        m = masks[0] if shared else masks[f]
        key = (id(frames[f]), 0 if shared else f % len(masks))
        if key not in want:
            want[key] = frames[f].extract(m)
        _assert_same_result(int(n[f]), k[f, :n[f]], d[f, :n[f]], *want[key])


def test_cpp_adapter(gpu, oracle, tmp_path):
    """tests/cpp/orb_mask_adapter.cpp: ORB_SLAM3::ORBextractor::honourMask and the masked dvslam::OrbExtractor overload"""
    exe = os.path.join(str(tmp_path), "orb_mask_adapter")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "tests", "cpp", "stubs"), os.path.join(ROOT, "tests", "cpp", "orb_mask_adapter.cpp"), "-o", exe,
                           "-L" + LIBDIR, "-ldvslam_hip", "-Wl,-rpath," + LIBDIR, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    r = _ref(oracle, 3)
    mask = make_mask("boxes", seed=3)
    src = os.path.join(str(tmp_path), "in.bin"); dst = os.path.join(str(tmp_path), "out.txt")
    with open(src, "wb") as f:
        f.write(np.array([ROWS, COLS], np.int32).tobytes() + r.img.tobytes() + mask.tobytes())
    p = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    got, flags = {}, {}
    lines = open(dst).read().splitlines()
    i = 0
    while i < len(lines):
        w = lines[i].split()
        if w[0] == "BEGIN":
            rows = [lines[i + 1 + j].split() for j in range(int(w[2]))]
            got[w[1]] = rows
            i += 1 + len(rows)
        else:
            flags[w[0]] = int(w[1])
            i += 1

    def as_rows(res):
        n, k, d = res
        return [[f"{int(k[f].view(np.uint32)[j]):08x}" for f in ("x", "y", "size", "angle", "response")] +
                [str(int(k["octave"][j])), str(int(k["class_id"][j])), d[j].tobytes().hex()] for j in range(n)]

    masked = r.extract(mask)
    assert got["off"] == as_rows(r.result)
    assert got["on"] == as_rows(masked)
    assert got["on_nomask"] == as_rows(r.result)
    assert got["raw"] == as_rows(masked)
    assert flags == {"THROWS": 3, "BADSTEP": 1}
