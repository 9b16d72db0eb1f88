"""dvs_motion_* on the GPU (csrc/motion_seg.hip) against tests/motion_ref.py, bit for bit: the seed image and n_valid on scene 1 with the
rule's edges in the inputs (each asserted to be there), labels and areas through the labelling hook on patterns built against the tile
structure, the mask and every statistic at the area threshold and the radius limits, host form against device form, repeatability, no
state from one call in the next, and the composition with the masked extractor."""
import numpy as np
import pytest
import motion_ref as mr

GATES = [299, 300, 301, 2999, 3000, 3001]
CASES = ["fwd", "back", "same", "rot100"]


def _segmenter(rows, cols, K, **kw):
    from dvslam_amd import motion as M
    return M.MotionSegmenter(M.default_params(rows, cols, *K, **kw), hooks=True)


def _inverse(R, t):
    return R.T.copy(), -(R.T @ t)


def _seed_inputs(cols, rows, which):
    """scene 1 from the reference camera (the world frame) and from the current one, with the rule's edges written into both images"""
    R, t = mr.SCENE1_MOTION
    if which == "back":
        R, t = _inverse(R, t)
    if which == "same":                             # the identity: pixel (u, v) projects onto (u, v), every border row and column is hit
        R, t = np.eye(3), np.zeros(3)
    box = (-0.35, -0.15, 0.25, 0.3, 1.0)            # a box face that moves by more than its width between the two images: seeds in bulk
    Dr = mr.scene1_depth(cols, rows, None, None, box)
    Dc = mr.scene1_depth(cols, rows, R, t, (box[0] + 0.3,) + box[1:])
    if which == "rot100":
        R = mr.rot("y", 100.0)
    K = mr.scene1_K(cols, rows)
    Dr[rows // 2, cols // 4:cols // 4 + 6] = GATES                     # the gates and 1 mm either side, in windows the far plane's pixels look at ...
    Dc[2, 3:9] = GATES                              # ... and in the current image
    Dr[rows // 3, cols // 3] = 0                    # one invalid pixel inside otherwise valid windows
    # a run of current pixels whose residual against the reference lies within 1 mm of tau, on either side in turn: the depth is estimated
    # from zr = z g + t[2] (g: the ray under R's third row) solved for zr = m / 1000 - tau(zr), then the reference itself picks, among the
    # 13 depths around the estimate, the one whose margin is the smallest positive / the largest non-positive
    base = mr.seeds(Dr, Dc, K, R, t)[2]
    v0 = (2 * rows) // 3
    fx, fy, cx, cy = K
    run = [c for c in range(cols // 8, cols // 8 + 14) if base["reached"][v0, c]]
    est = {}
    for c in run:
        g = R[2, 0] * (c - cx) / fx + R[2, 1] * (v0 - cy) / fy + R[2, 2]
        zr = base["m"][v0, c] * 0.001
        for _ in range(4):
            zr = base["m"][v0, c] * 0.001 - (mr.DEFAULTS["tau0_m"] + mr.DEFAULTS["tau2_per_m"] * zr * zr)
        est[c] = int(round((zr - t[2]) / g * 1000.0))
    margins = {}
    for k in range(-6, 7):
        trial = Dc.copy()
        for c in run:
            trial[v0, c] = est[c] + k
        a = mr.seeds(Dr, trial, K, R, t)[2]
        margins[k] = {c: (a["margin"][v0, c] if a["reached"][v0, c] else np.nan) for c in run}
    for i, c in enumerate(run):
        ks = [k for k in margins if (margins[k][c] > 0 if i % 2 else margins[k][c] <= 0)]
        if ks:
            Dc[v0, c] = est[c] + min(ks, key=lambda k: abs(margins[k][c]))
    return Dr, Dc, K, R, t


@pytest.fixture(scope="module")
def seed_cases():
    """inputs and reference results, computed once per size and left unchanged"""
    out = {}
    for cols, rows in ((320, 240), (63, 65)):
        for which in CASES:
            Dr, Dc, K, R, t = _seed_inputs(cols, rows, which)
            kw = dict(min_area=200 if cols > 100 else 12)
            out[(cols, rows, which)] = (Dr, Dc, K, R, t, kw, mr.segment(Dr, Dc, K, R, t, **kw))
    return out


@pytest.mark.parametrize("size", [(320, 240), (63, 65)], ids=["320x240", "63x65"])
def test_inputs_contain_the_rules_edges(seed_cases, size):
    """no GPU work: what the seed test below relies on is in its inputs"""
    cols, rows = size
    ur_seen, vr_seen = set(), set()
    for which in CASES:
        Dr, Dc, K, R, t, kw, want = seed_cases[(cols, rows, which)]
        a = want["aux"]
        assert np.isin(GATES, Dc).all() and np.isin(GATES, Dr).all()
        f = a["front"]
        ur_seen |= set(a["ur"][f].astype(np.int64).tolist()); vr_seen |= set(a["vr"][f].astype(np.int64).tolist())
        if which == "rot100":
            assert (a["cur_ok"] & (a["zr"] <= 0)).sum() > rows and f.sum() > rows          # zr <= 0 under the 100 degree rotation, and not everywhere
            continue
        ins = a["inside"]
        # every gate value of the reference lies in a window that some pixel examines
        for g in GATES:
            near = np.zeros((rows, cols), bool)
            ys, xs = np.nonzero(Dr == g)
            for y, x in zip(ys, xs):
                near |= ins & (abs(a["iv"] - y) <= 1) & (abs(a["iu"] - x) <= 1)
            assert near.any(), (which, g)
        assert (ins & (a["n_win_invalid"] == 1)).any(), which                                # one invalid pixel in an otherwise valid 3 x 3
        r = a["reached"]
        assert (r & (a["margin"] > 0) & (a["margin"] < 1e-3)).any() and (r & (a["margin"] <= 0) & (a["margin"] > -1e-3)).any(), which
        assert want["stats"]["n_valid"] > rows * cols // 2 and want["stats"]["n_dynamic"] > rows * cols // 20
    assert {0, 1, cols - 2, cols - 1} <= ur_seen and {0, 1, rows - 2, rows - 1} <= vr_seen


@pytest.mark.gpu
@pytest.mark.parametrize("which", CASES)
@pytest.mark.parametrize("size", [(320, 240), (63, 65)], ids=["320x240", "63x65"])
def test_seeds_and_n_valid_bit_for_bit(gpu, hooks, seed_cases, size, which):
    """device form with row steps larger than the rows; the padding of the mask stays untouched"""
    from dvslam_amd._lib import DeviceBuffer
    cols, rows = size
    Dr, Dc, K, R, t, kw, want = seed_cases[(cols, rows, which)]
    seg = _segmenter(rows, cols, K, **kw)
    rs, cs, ms = cols * 2 + 6, cols * 2 + 64, cols + 5
    pr = np.full((rows, rs // 2), 1234, np.uint16); pr[:, :cols] = Dr
    pc = np.full((rows, cs // 2), 1234, np.uint16); pc[:, :cols] = Dc
    pm = np.full((rows, ms), 0x77, np.uint8)
    d_r, d_c, d_m = DeviceBuffer(pr.nbytes).upload(pr), DeviceBuffer(pc.nbytes).upload(pc), DeviceBuffer(pm.nbytes).upload(pm)
    st = seg.segment_device(d_r, rs, d_c, cs, R, t, d_m, ms, want_stats=True)
    seed, lab, dyn = seg.stages()
    got = d_m.download(np.uint8, pm.size).reshape(rows, ms)
    print(size, which, st)
    assert (seed.astype(bool) == want["seed"]).all()
    assert st["n_valid"] == want["stats"]["n_valid"] and st["n_seed"] == want["stats"]["n_seed"]
    assert (lab == want["labels"]).all() and (dyn.astype(bool) == want["dynamic"]).all()
    assert (got[:, :cols] == want["mask"]).all() and (got[:, cols:] == 0x77).all()
    assert st == want["stats"]
    # the host form on strided views of the same arrays
    mask, st2 = seg.segment(pr[:, :cols], pc[:, :cols], R, t)
    assert (mask == want["mask"]).all() and st2 == want["stats"]
    for b in (d_r, d_c, d_m):
        b.free()
    seg.close()


@pytest.mark.gpu
@pytest.mark.parametrize("size", mr.LABEL_SIZES, ids=lambda s: "%dx%d" % (s[1], s[0]))
def test_labels_and_areas_on_every_pattern(gpu, hooks, size):
    from dvslam_amd import motion as M
    rows, cols = size
    n = 0
    for name, img in mr.patterns(rows, cols):
        lab, area = M.label_image(img)
        want = mr.labels_scipy(img)
        assert (lab == want).all(), name
        assert (area == mr.areas(want)).all(), name
        n += 1
    assert n == 11


@pytest.mark.gpu
def test_labels_across_many_workgroups(gpu, hooks):
    """720 x 1280: 920 tiles, more workgroups than one XCD takes — the merge across tile borders with every XCD at work"""
    from dvslam_amd import motion as M
    by = dict(mr.patterns(720, 1280))
    for name in ("full", "every_tile", "comb", "random0.5", "random0.6"):
        lab, area = M.label_image(by[name])
        want = mr.labels_scipy(by[name])
        assert (lab == want).all() and (area == mr.areas(want)).all(), name


def _blob_scene(rows, cols, blobs):
    """reference: a wall at 2 m; current: the same with blobs at 1 m; identity pose -> the seeds are exactly the blobs (off the border)"""
    Dr = np.full((rows, cols), 2000, np.uint16)
    Dc = Dr.copy()
    for y0, y1, x0, x1 in blobs:
        Dc[y0:y1, x0:x1] = 1000
    return Dr, Dc


@pytest.mark.gpu
@pytest.mark.parametrize("radius", [0, 1, 31])
def test_mask_and_statistics_at_the_area_threshold(gpu, hooks, radius):
    rows, cols, min_area = 100, 150, 50
    K = (120.0, 120.0, 74.5, 49.5)
    # a blob in every corner, as near the border as a seed can be (row / column 1): 50 px kept, 49 px dropped, an L of 50 kept, 49 dropped
    blobs = [(1, 6, 1, 11), (1, 8, cols - 8, cols - 1), (rows - 11, rows - 1, 1, 5), (rows - 3, rows - 1, 5, 10), (rows - 8, rows - 1, cols - 8, cols - 1),
             (40, 47, 60, 67), (50, 55, 60, 70)]
    Dr, Dc = _blob_scene(rows, cols, blobs)
    want = mr.segment(Dr, Dc, K, np.eye(3), np.zeros(3), min_area=min_area, dilate_radius=radius)
    sizes = sorted(want["area"][want["area"] > 0].tolist())
    assert sizes == [49, 49, 49, 50, 50, 50] and want["stats"]["n_components_kept"] == 3
    assert (want["mask"][0, 0], want["mask"][rows - 1, 0], want["mask"][0, cols - 1]) == ((0, 0, 255) if radius else (255, 255, 255))
    seg = _segmenter(rows, cols, K, min_area=min_area, dilate_radius=radius)
    mask, st = seg.segment(Dr, Dc, np.eye(3), np.zeros(3))
    seed, lab, dyn = seg.stages()
    print(radius, st)
    assert (seed.astype(bool) == want["seed"]).all() and (lab == want["labels"]).all() and (dyn.astype(bool) == want["dynamic"]).all()
    assert (mask == want["mask"]).all() and st == want["stats"]
    assert st["n_masked"] == ((mask == 0).sum()) and st["n_dynamic"] == 150
    seg.close()


@pytest.mark.gpu
def test_entry_points_repeatability_and_no_state_between_calls(gpu, hooks):
    from dvslam_amd._lib import DeviceBuffer, DvsError
    rows, cols = 97, 131
    K = (110.0, 110.0, 65.0, 48.0)
    full = _blob_scene(rows, cols, [(0, rows, 0, cols)])
    some = _blob_scene(rows, cols, [(10, 40, 20, 60), (70, 90, 100, 125)])
    empty = _blob_scene(rows, cols, [])
    I, z = np.eye(3), np.zeros(3)
    seg = _segmenter(rows, cols, K, min_area=20, dilate_radius=3)
    d_r, d_c, d_m = DeviceBuffer(rows * cols * 2), DeviceBuffer(rows * cols * 2), DeviceBuffer(rows * cols)

    def device(scene):
        d_r.upload(scene[0]); d_c.upload(scene[1]); d_m.upload(np.full(rows * cols, 0x55, np.uint8))
        st = seg.segment_device(d_r, cols * 2, d_c, cols * 2, I, z, d_m, cols, want_stats=True)
        return d_m.download(np.uint8, rows * cols).reshape(rows, cols), st
    want = mr.segment(*some, K, I, z, min_area=20, dilate_radius=3)
    m1, s1 = device(some)
    m2, s2 = device(some)
    mh, sh = seg.segment(*some, I, z)
    assert m1.tobytes() == m2.tobytes() == mh.tobytes() == want["mask"].tobytes() and s1 == s2 == sh == want["stats"]
    assert s1["n_components_kept"] == 2 and s1["n_masked"] > s1["n_dynamic"] > 0
    # everything dynamic, then nothing: labels, areas and counters of the full call must not show in the empty one
    mf, sf = device(full)
    assert sf["n_seed"] == (rows - 2) * (cols - 2) and sf["n_components"] == 1 and (mf == 0).all() and sf["n_masked"] == rows * cols
    me, se = device(empty)
    assert (me == 255).all() and se == dict(n_valid=(rows - 2) * (cols - 2), n_seed=0, n_components=0, n_components_kept=0, n_dynamic=0, n_masked=0)
    seed, lab, dyn = seg.stages()
    assert not seed.any() and (lab == -1).all() and not dyn.any()
    m3, s3 = device(some)
    assert m3.tobytes() == m1.tobytes() and s3 == s1
    # argument errors with a handle in hand: a pose that is not finite, steps below the row
    bad = I.copy(); bad[1, 1] = np.nan
    for args in ((d_r, cols * 2, d_c, cols * 2, bad, z, d_m, cols), (d_r, cols * 2, d_c, cols * 2, I, np.array([0, np.inf, 0]), d_m, cols),
                 (d_r, cols * 2 - 2, d_c, cols * 2, I, z, d_m, cols), (d_r, cols * 2, d_c, cols * 2 + 1, I, z, d_m, cols),
                 (d_r, cols * 2, d_c, cols * 2, I, z, d_m, cols - 1)):
        with pytest.raises(DvsError) as e:
            seg.segment_device(*args)
        assert e.value.code == -6
    for b in (d_r, d_c, d_m):
        b.free()
    seg.close()


@pytest.mark.gpu
def test_produced_mask_keeps_keypoints_off_the_moving_block(gpu):
    """composition with the extractor: extract_masked with a produced mask puts no keypoint on a zero pixel"""
    from dvslam_amd import ORBextractor, motion as M
    frames, depths, boxes = mr.scene2(5)
    rows, cols = depths[0].shape
    seg = M.MotionSegmenter(M.default_params(rows, cols, 600.0, 600.0, cols / 2.0, rows / 2.0))
    flat = np.full((rows, cols), 1500, np.uint16)
    mask, st = seg.segment(flat, depths[4], np.eye(3), np.zeros(3))
    x0, y0, w, h = boxes[4]
    assert st["n_components_kept"] == 1 and (mask[y0:y0 + h, x0:x0 + w] == 0).all() and 0 < (mask == 0).sum() < rows * cols // 3
    orb = ORBextractor(1000, 1.2, 8, 20, 7)
    n0, k0, _ = orb(frames[4])
    n, k, _ = orb.extract_masked(frames[4], mask)
    xi, yi = np.floor(k["x"]).astype(np.int64), np.floor(k["y"]).astype(np.int64)
    assert n > 500 and (mask[yi, xi] != 0).all()
    assert (mask[np.floor(k0["y"]).astype(np.int64), np.floor(k0["x"]).astype(np.int64)] == 0).sum() >= 20   # the mask had something to do
    seg.close()
