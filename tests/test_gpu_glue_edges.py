"""csrc/frontend.hip's kernels (and the compaction / scan kernels of csrc/match.hip behind the association) against the numpy statements
of tests/glue_ref.py, on scenes with a keypoint on every gate, rounding rule and trip edge (their preconditions are asserted on the CPU,
tests/test_glue_ref_cpu.py).  Every output is integer or exactly rounded: all comparisons are on byte patterns, no tolerance.  Output
buffers are pre-filled with a sentinel byte and everything outside the promised region must still hold it afterwards."""
import numpy as np
import pytest
import glue_ref as gr
from dvslam_amd._lib import KP_DTYPE

pytestmark = pytest.mark.gpu
SENT = 0xA5
KPB = KP_DTYPE.itemsize


@pytest.fixture(scope="module")
def g(gpu):
    from dvslam_amd import FrontendGlue
    return FrontendGlue()


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _sent(shape, dtype):
    a = np.empty(shape, dtype)
    a.view(np.uint8).reshape(-1)[:] = SENT
    return a


def _untouched(a):
    return bool((np.ascontiguousarray(a).view(np.uint8) == SENT).all())


def _dev(arr=None, nbytes=None):
    """device buffer holding arr, or nbytes of sentinel"""
    from dvslam_amd._lib import DeviceBuffer
    if arr is None:
        arr = np.full(max(nbytes, 16), SENT, np.uint8)
    arr = np.ascontiguousarray(arr)
    return DeviceBuffer(max(arr.nbytes, 16)).upload(arr)


# ------------------------------------------------------------------------------------------------ depth gate
FORMS = ((True, True), (False, True), (True, False), (False, False))      # (descriptors, out_index)


def _check_filter_depth(g, kps, desc, depth, gate, with_desc, with_index, what):
    n = len(kps)
    ref = gr.depth_gate(kps, depth, *gate)
    out = (_sent(n, KP_DTYPE), _sent((n, 32), np.uint8), _sent(n, np.int32))
    ok, od, oi = g.filter_depth(kps, desc if with_desc else None, depth, *gate, with_index=with_index, out=out)
    m = len(ok)
    assert m == len(ref), what
    assert _bits(ok) == _bits(kps[ref]) and _untouched(out[0][m:]), what
    assert (_bits(od) == _bits(desc[ref]) and _untouched(out[1][m:])) if with_desc else _untouched(out[1]), what
    assert (_bits(oi) == _bits(ref) and _untouched(out[2][m:])) if with_index else _untouched(out[2]), what


@pytest.mark.parametrize("pattern", gr.PATTERNS)
def test_filter_depth_counts_and_keep_patterns(g, pattern):
    """every count either side of a 256-chunk and of a 1024-trip, with the keep patterns that stress the carried offset"""
    for i, n in enumerate(gr.N1024):
        kps, desc, depth, _ = gr.pattern_scene(n, pattern)
        for form in {FORMS[0], FORMS[1 + i % 3]}:
            _check_filter_depth(g, kps, desc, gr.padded(depth, 6) if i % 2 else depth, gr.GATES["default"], *form, (pattern, n, form))


@pytest.mark.parametrize("gate", list(gr.GATES))
def test_filter_depth_gates_and_rounding(g, gate):
    """keypoints on the planted depths either side of both gates, on the rounding rule and across the image border"""
    kps, desc, depth, _ = gr.edge_scene()
    for form in FORMS:
        for d in (depth, gr.padded(depth, 6)):                             # host step_bytes = 2 * cols + 6
            assert d.strides[0] == 2 * gr.COLS + (0 if d is depth else 6)
            _check_filter_depth(g, kps, desc, d, gr.GATES[gate], *form, (gate, form))


@pytest.mark.parametrize("shared_image", [False, True])
def test_filter_depth_batch_device(g, shared_image):
    """six frames of 300 rows: counts 0, 1, 257, the full stride, one past it and a negative one (both clamped); a padded depth image per
    frame, or one image for all (frame stride 0); with and without descriptors / indices"""
    kps, desc, depth, counts = gr.batch_scene()
    F, S = kps.shape
    step = 2 * gr.COLS + 6
    fstride = gr.ROWS * step + 2
    zbuf = np.full(F * fstride, 0xEE, np.uint8)
    for f in range(F):
        np.ndarray((gr.ROWS, gr.COLS), np.uint16, zbuf, f * fstride, (step, 2))[:] = depth[f]
    d_k, d_d, d_n, d_z = _dev(kps), _dev(desc), _dev(counts), _dev(zbuf)
    for with_desc, with_index in FORMS[:3]:
        o_k, o_d, o_i, o_n = _dev(nbytes=F * S * KPB), _dev(nbytes=F * S * 32), _dev(nbytes=F * S * 4), _dev(nbytes=F * 4)
        g.filter_depth_batch_device(d_k.ptr, d_d.ptr if with_desc else None, d_n.ptr, S, F, d_z.ptr, gr.ROWS, gr.COLS, step,
                                    0 if shared_image else fstride, o_k.ptr, o_d.ptr, o_i.ptr if with_index else None, o_n.ptr)
        g.synchronize()
        ok = o_k.download(KP_DTYPE, F * S).reshape(F, S); od = o_d.download(np.uint8, F * S * 32).reshape(F, S, 32)
        oi = o_i.download(np.int32, F * S).reshape(F, S); on = o_n.download(np.int32, F)
        for f, n in enumerate(gr.batch_effective_counts()):
            ref = gr.depth_gate(kps[f, :n], depth[0 if shared_image else f])
            m = len(ref)
            what = (shared_image, with_desc, with_index, f)
            assert on[f] == m, what
            assert _bits(ok[f, :m]) == _bits(kps[f, ref]) and _untouched(ok[f, m:]), what
            assert (_bits(od[f, :m]) == _bits(desc[f, ref]) and _untouched(od[f, m:])) if with_desc else _untouched(od[f]), what
            assert (_bits(oi[f, :m]) == _bits(ref) and _untouched(oi[f, m:])) if with_index else _untouched(oi[f]), what


# ------------------------------------------------------------------------------------------------ distance filter
def test_filter_matches_edges_counts_and_patterns(g):
    for n in gr.N256:
        cases = [(gr.match_scene(n), maxd) for maxd in gr.MATCH_MAXD] + [(gr.match_scene(n, p), 50.0) for p in gr.PATTERNS]
        for (idx, dist), maxd in cases:
            ref = gr.filter_matches(idx, dist, maxd)
            out = _sent((n, 3), np.int32)
            got = g.filter_matches(idx, dist, maxd, out=out)
            assert len(got) == len(ref) and _bits(got) == _bits(ref) and _untouched(out[len(ref):]), (n, maxd)


# ------------------------------------------------------------------------------------------------ back-projection, payload
Q = (0.0, 0.0, float(np.sqrt(0.5)), float(np.sqrt(0.5)))
FRAME_IDS = ["", "a", "ab", "abc", "abcd", "abcde", "abcdef", "abcdefg", "f" * 63]


def test_backproject_counts_gates_and_rounding(g):
    for i, n in enumerate(gr.N256):
        kps, desc, depth, _ = gr.edge_scene(n)
        w, oi = gr.backproject(kps, depth, *gr.INTRINSICS, gr.R_GENERAL, gr.T_GENERAL)
        out = (_sent((n, 3), np.float64), _sent(n, np.int32))
        w2, oi2 = g.backproject(kps, gr.padded(depth, 6) if i % 2 else depth, *gr.INTRINSICS, gr.R_GENERAL, gr.T_GENERAL, out=out)
        m = len(oi)
        assert len(oi2) == m and _bits(oi2) == _bits(oi) and _bits(w2.view(np.uint64)) == _bits(w.view(np.uint64)), n
        assert _untouched(out[0][m:]) and _untouched(out[1][m:]), n


def test_publish_keyframe_host_payload_bytes(g):
    from dvslam_amd import DvsError
    from dvslam_amd._lib import lib
    args = gr.INTRINSICS + (gr.R_GENERAL, gr.T_GENERAL)
    kps, desc, depth, _ = gr.edge_scene(257)
    for fid in FRAME_IDS:                                        # every alignment phase of the uint64 behind the string, and the longest
        want, m = gr.keyframe_payload(kps, desc, depth, *args, (12, 345678), fid, 77, Q)
        got, m2 = g.publish_keyframe(kps, desc, gr.padded(depth, 6), *args, (12, 345678), fid, 77, Q)
        assert m2 == m and got == want, fid
    with pytest.raises(DvsError) as e:
        g.publish_keyframe(kps, desc, depth, *args, frame_id="f" * 64)
    assert e.value.code == -6                                    # DVS_ERR_ARG
    for n in gr.N256:
        kps, desc, depth, _ = gr.edge_scene(n)
        want, m = gr.keyframe_payload(kps, desc, depth, *args)
        got, m2 = g.publish_keyframe(kps, desc, depth, *args)
        assert m2 == m and got == want, n
        if n:
            with pytest.raises(DvsError) as e:
                g.publish_keyframe(kps, desc, depth, *args, cap=len(want) - 1)
            assert e.value.code == -3 and e.value.needed == len(want), n       # DVS_ERR_CAPACITY, the needed size reported
    kps, desc, depth, _ = gr.edge_scene(257)
    want, m = gr.keyframe_payload(kps, desc, np.zeros_like(depth), *args)
    assert m == 0 and g.publish_keyframe(kps, desc, np.zeros_like(depth), *args) == (want, 0)      # m = 0 with n > 0
    one = gr.edge_scene(1)
    want, m = gr.keyframe_payload(*one[:3], *args)
    assert m == 1 and len(want) == lib().dvs_keyframe_cdr_capacity(b"camera_link", 1)              # m = 1: no trailing pad
    assert g.publish_keyframe(*one[:3], *args) == (want, 1)


def test_publish_keyframe_device_form(g):
    """device-resident inputs, padded depth rows; nothing behind the payload is written, and nothing at all when it does not fit"""
    from dvslam_amd._lib import lib
    args = gr.INTRINSICS + (gr.R_GENERAL, gr.T_GENERAL)
    for n, fid, zero in ((1, "camera_link", False), (257, "abc", False), (513, "", False), (255, "camera_link", True)):
        kps, desc, depth, _ = gr.edge_scene(n)
        if zero:
            depth = np.zeros_like(depth)
        want, m = gr.keyframe_payload(kps, desc, depth, *args, (3, 4), fid, 9, Q)
        z = gr.padded(depth, 10)
        cap = lib().dvs_keyframe_cdr_capacity(fid.encode(), n)
        assert len(want) <= cap
        d_k, d_d, d_z = _dev(kps), _dev(desc), _dev(z.base)
        for short in (False, True):
            this_cap = len(want) - 1 if short else cap
            d_o, d_s, d_m = _dev(nbytes=cap + 64), _dev(nbytes=8), _dev(nbytes=4)
            g.publish_keyframe_device(d_k.ptr, d_d.ptr, n, d_z.ptr, gr.ROWS, gr.COLS, z.strides[0], *gr.INTRINSICS, gr.R_GENERAL, gr.T_GENERAL,
                                      d_o.ptr, this_cap, d_s.ptr, d_m.ptr, (3, 4), fid, 9, Q)
            g.synchronize()
            out = d_o.download(np.uint8, cap + 64)
            assert d_s.download(np.uint64, 1)[0] == len(want) and d_m.download(np.int32, 1)[0] == m, (n, short)
            if short:
                assert _untouched(out), n
            else:
                assert out[:len(want)].tobytes() == want and _untouched(out[len(want):]), n


# ------------------------------------------------------------------------------------------------ gray
def _bgr_padded(img, p):
    rows, cols, _ = img.shape
    step = 3 * cols + p
    buf = np.full(rows * step, 0xEE, np.uint8)
    view = np.ndarray((rows, cols, 3), np.uint8, buf, 0, (step, 3, 1))
    view[:] = img
    return view


@pytest.mark.parametrize("variant", [0, 1])
def test_bgr_to_gray_host_shapes(g, variant):
    i = 0
    for rows in gr.GRAY_ROWS:
        for cols in gr.GRAY_COLS:
            img = gr.gray_scene(rows, cols, 3)[i % 3]
            gs = cols + (0, 1, 3)[i % 3]
            out = _sent((rows, gs), np.uint8)
            g.bgr_to_gray(_bgr_padded(img, i % 4), variant, out=out[:, :cols])
            assert _bits(out[:, :cols]) == _bits(gr.gray(img, variant)) and _untouched(out[:, cols:]), (rows, cols)
            i += 1


@pytest.mark.parametrize("variant", [0, 1])
def test_bgr_to_gray_device_form(g, variant):
    """three frames per call; input rows padded by 0 .. 3 bytes, gray rows by 0, 1 or 3, frame strides that are no multiple of 4: the
    padding between gray rows and between frames stays untouched"""
    i = 0
    seen = set()
    for rows in gr.GRAY_ROWS:
        for cols in gr.GRAY_COLS:
            p, q = i % 4, (0, 1, 3)[i % 3]
            seen.add((p, q)); i += 1
            img = gr.gray_scene(rows, cols, 3)
            step, gstep = 3 * cols + p, cols + q
            fs = rows * step + 1; fs += fs % 4 == 0
            gfs = rows * gstep + 2; gfs += gfs % 4 == 0
            assert fs % 4 and gfs % 4
            src = np.full(3 * fs, 0xEE, np.uint8)
            for f in range(3):
                np.ndarray((rows, cols, 3), np.uint8, src, f * fs, (step, 3, 1))[:] = img[f]
            d_s, d_g = _dev(src), _dev(nbytes=3 * gfs)
            g.bgr_to_gray_device(d_s.ptr, 3, rows, cols, step, fs, d_g.ptr, gstep, gfs, variant)
            g.synchronize()
            out = d_g.download(np.uint8, 3 * gfs)
            written = np.zeros(3 * gfs, bool)
            for f in range(3):
                v = np.ndarray((rows, cols), np.uint8, out, f * gfs, (gstep, 1))
                assert _bits(v) == _bits(gr.gray(img[f], variant)), (rows, cols, f)
                np.ndarray((rows, cols), bool, written, f * gfs, (gstep, 1))[:] = True
            assert (out[~written] == SENT).all(), (rows, cols)
    assert len(seen) == 12


# ------------------------------------------------------------------------------------------------ Harris
def test_harris_host_every_pixel_and_outside(g):
    img, xs, ys = gr.harris_scene()
    for bs in gr.HARRIS_BLOCKS:
        got = g.harris_responses(img, xs, ys, bs)
        assert _bits(got.view(np.uint32)) == _bits(gr.harris_reference(bs).view(np.uint32)), bs
    wide = np.full((gr.HARRIS_ROWS, gr.HARRIS_COLS + 5), 0xEE, np.uint8); wide[:, :gr.HARRIS_COLS] = img
    assert _bits(g.harris_responses(wide[:, :gr.HARRIS_COLS], xs, ys, 7)) == _bits(gr.harris_reference(7))


def test_harris_device_form_padded_step(g):
    img, xs, ys = gr.harris_scene()
    step = gr.HARRIS_COLS + 5
    wide = np.full((gr.HARRIS_ROWS, step), 0xEE, np.uint8); wide[:, :gr.HARRIS_COLS] = img
    n = len(xs)
    d_i, d_x, d_y = _dev(wide), _dev(xs), _dev(ys)
    for bs in gr.HARRIS_BLOCKS:
        d_r = _dev(nbytes=4 * n + 64)
        g.harris_responses_device(d_i.ptr, gr.HARRIS_ROWS, gr.HARRIS_COLS, step, d_x.ptr, d_y.ptr, n, d_r.ptr, bs)
        g.synchronize()
        out = d_r.download(np.uint8, 4 * n + 64)
        assert out[:4 * n].tobytes() == _bits(gr.harris_reference(bs)) and _untouched(out[4 * n:]), bs


# ------------------------------------------------------------------------------------------------ association
def _scene_args(s):
    return (s["obs_desc"], s["obs_px"], s["lm_desc"], s["lm_xyz"], s["R"], s["t"]) + tuple(s["K"])


def test_association_hamming_gate(g):
    """pairs at Hamming 0, 49, 50, 51 and 256 under integer and non-integer gates (the gate is the ceil of the double)"""
    s = gr.assoc_exact_scene()
    for md in gr.ASSOC_MAX_DESC:
        best, offs, cand = gr.assoc_reference("exact", max_desc=md)
        assert _bits(g.associate(*_scene_args(s), max_desc=md)) == _bits(best), md
        b2, o2, c2 = g.associate_candidates(*_scene_args(s), max_desc=md)
        assert _bits(b2) == _bits(best) and _bits(o2) == _bits(offs) and _bits(c2) == _bits(cand), md


def test_association_reprojection_gate_ties_and_landmarks_behind(g):
    s = gr.assoc_exact_scene()
    obs, lm = s["obs"], s["lm"]
    for mr in (5.0, float(np.nextafter(5.0, np.inf)), 2.5, 1.0):
        ref = gr.assoc_reference("exact", max_reproj=mr)[0]
        got = g.associate(*_scene_args(s), max_reproj=mr)
        assert _bits(got) == _bits(ref), mr
    got = g.associate(*_scene_args(s))
    assert got[obs["axis"]] == -1 and got[obs["tie"]] == lm["tie_a"] and got[obs["later"]] == lm["later_near"]
    assert got[obs["behind_hit"]] == lm["behind"] and got[obs["plane_hit"]] == lm["plane"] and got[obs["plane_miss"]] == -1
    assert g.associate(*_scene_args(s), max_reproj=float(np.nextafter(5.0, np.inf)))[obs["axis"]] == lm["axis"]


@pytest.mark.parametrize("nobs,nlm", gr.ASSOC_SIZES)
def test_association_counts(g, nobs, nlm):
    """observation counts either side of the scan's 1024 threads and of a workgroup's four wavefronts, landmark counts either side of
    a wavefront's 64-row trip; best matches, candidate offsets and candidate lists"""
    from dvslam_amd import DvsError
    s = gr.assoc_sweep_scene(nobs, nlm)
    best, offs, cand = gr.assoc_reference("sweep", nobs, nlm)
    assert _bits(g.associate(*_scene_args(s))) == _bits(best)
    b2, o2, c2 = g.associate_candidates(*_scene_args(s))
    assert _bits(b2) == _bits(best) and _bits(o2) == _bits(offs) and _bits(c2) == _bits(cand)
    if len(cand):
        with pytest.raises(DvsError) as e:
            g.associate_candidates(*_scene_args(s), cand_cap=len(cand) - 1)
        assert e.value.code == -3 and e.value.n_cand == len(cand)              # DVS_ERR_CAPACITY, the needed entries reported
    for md in (0.0, 1000.0):                                                    # no candidate at all / every pair a candidate
        best, offs, cand = gr.assoc_reference("sweep", nobs, nlm, max_desc=md)
        b2, o2, c2 = g.associate_candidates(*_scene_args(s), max_desc=md)
        assert len(cand) == (nobs * nlm if md else 0)
        assert _bits(b2) == _bits(best) and _bits(o2) == _bits(offs) and _bits(c2) == _bits(cand), md
