"""tests/glue_ref.py on the CPU: its numpy statements equal the C++ oracle bit for bit on every scene the GPU edge tests use, and
every scene really contains the edges it is there for (a scene without its edge fails HERE; it must not pass silently on the GPU)."""
import numpy as np
import pytest
import glue_ref as gr

F32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


# ------------------------------------------------------------------------------------------------ the rounding rule
def test_round_px_is_std_round():
    v = np.array([10.5, gr.nextafter0(10.5), 11.5, 0.49999997, -0.4, -0.5, -0.49999997, 39.5, gr.nextafter0(39.5), 1e5, -1.5, 0.0, 8388609.0], F32)
    assert gr.round_px(v).tolist() == [11, 10, 12, 0, 0, -1, 0, 40, 39, 100000, -2, 0, 8388609]
    assert np.floor(np.abs(F32(0.49999997)) + F32(0.5)) == 1.0           # the float32 shortcut is wrong exactly there
    assert np.rint(F32(10.5)) == 10.0                                    # and half-to-even differs at every even k + 0.5


# ------------------------------------------------------------------------------------------------ depth gate
def test_depth_scene_contains_its_edges():
    kps, desc, depth, classes = gr.edge_scene()
    planted = dict(zip(gr.PLANTED_DEPTHS, gr.gate_verdict(np.array(gr.PLANTED_DEPTHS, np.uint16)).tolist()))
    assert planted == {0: False, 299: False, 300: True, 301: True, 2999: True, 3000: False, 3001: False, 65535: False,
                       999: True, 1000: True, 1001: True}                # 300 * 0.001f = 0.3f is kept, 3000 * 0.001f = 3.0000002f is not
    a, b = classes["planted"]
    assert b <= len(kps) and depth[gr.round_px(kps["y"][a:b]), gr.round_px(kps["x"][a:b])].tolist() == list(gr.PLANTED_DEPTHS)
    assert gr.gate_verdict(depth[gr.KEEP_PX[1], gr.KEEP_PX[0]]) and not gr.gate_verdict(depth[gr.DROP_PX[1], gr.DROP_PX[0]])
    for name, (dmin, dmax) in gr.GATES.items():
        z = np.array(gr.PLANTED_DEPTHS, np.uint16).astype(F32) * F32(0.001)
        keep = set(gr.depth_gate(kps, depth, dmin, dmax).tolist()) & set(range(a, b))
        if name == "empty":
            assert dmin > dmax and len(gr.depth_gate(kps, depth, dmin, dmax)) == 0
            continue
        below = {a + i for i in range(b - a) if z[i] < F32(dmin)}; above = {a + i for i in range(b - a) if z[i] > F32(dmax)}
        assert keep and below and above and not (keep & (below | above)) and keep | below | above == set(range(a, b)), name
    # the rounding set: the two pixels either side of every half-way coordinate get different verdicts, the near side of every
    # border coordinate is kept somewhere, and the image border is crossed in both directions
    verdict = gr.gate_verdict(depth)
    kept = set(gr.depth_gate(kps, depth).tolist())
    for cls, axis, size in (("round_x", "x", gr.COLS), ("round_y", "y", gr.ROWS)):
        a, b = classes[cls]
        vals = kps[axis][a:b]
        assert set(vals.tolist()) == set(float(v) for v in gr.rounding_values(size))
        for i in range(a, b):
            v = kps[axis][i]; other = gr.round_px(kps["y" if axis == "x" else "x"][i])
            if v == np.floor(v) + F32(0.5) and 0 <= np.floor(v) and np.floor(v) + 1 < size:      # k + 0.5 inside the image
                k = int(np.floor(v))
                pair = verdict[other, k:k + 2] if axis == "x" else verdict[k:k + 2, other]
                assert pair[0] != pair[1], (cls, i)
        r = gr.round_px(vals)
        assert (r < 0).any() and (r >= size).any() and (r == 0).any() and (r == size - 1).any()
        for target in (0, size - 1, 10, 11, 12):                        # each rounded position is kept in one row / column, dropped in the other
            idx = [a + j for j in range(b - a) if r[j] == target]
            assert any(i in kept for i in idx) and any(i not in kept for i in idx), (cls, target)
        assert not any(a + j in kept for j in range(b - a) if r[j] < 0 or r[j] >= size)


def test_depth_gate_matches_oracle(oracle):
    kps, desc, depth, _ = gr.edge_scene()
    for name, (dmin, dmax) in gr.GATES.items():
        ok, od, oi = oracle.filter_depth(kps, desc, depth, dmin, dmax)
        ref = gr.depth_gate(kps, depth, dmin, dmax)
        assert _bits(oi) == _bits(ref) and _bits(ok) == _bits(kps[ref]) and _bits(od) == _bits(desc[ref]), name
    for f, n in enumerate(gr.batch_effective_counts()):
        bk, bd, bz, _ = gr.batch_scene()
        oi = oracle.filter_depth(bk[f, :n], bd[f, :n], bz[f])[2]
        assert _bits(oi) == _bits(gr.depth_gate(bk[f, :n], bz[f])), f


def test_pattern_scenes_contain_their_counts_and_patterns(oracle):
    assert set(gr.N1024) == {0, 1, 255, 256, 257, 513, 1023, 1024, 1025, 2049} and set(gr.N256) == {0, 1, 255, 256, 257, 513}
    for n in gr.N1024:
        for pattern in gr.PATTERNS:
            kps, desc, depth, mask = gr.pattern_scene(n, pattern)
            ref = gr.depth_gate(kps, depth)
            assert len(kps) == n and _bits(ref) == _bits(np.nonzero(mask)[0].astype(np.int32)), (n, pattern)
            assert _bits(oracle.filter_depth(kps, desc, depth)[2]) == _bits(ref)
    m = {p: gr.pattern_mask(1025, p) for p in gr.PATTERNS}
    assert m["all"].all() and not m["none"].any() and m["alternating"].sum() == 512 and m["last"].nonzero()[0].tolist() == [1024]
    assert m["chunk_first"].nonzero()[0].tolist() == [0, 256, 512, 768, 1024]


def test_batch_scene_contains_its_edges():
    kps, desc, depth, counts = gr.batch_scene()
    assert counts.tolist() == [0, 1, 257, 300, 309, -3] and gr.batch_effective_counts() == [0, 1, 257, 300, 300, 0]
    assert kps.shape == (6, gr.BATCH_STRIDE) and depth.shape == (6, gr.ROWS, gr.COLS)
    kept = [gr.depth_gate(kps[f, :n], depth[f]) for f, n in enumerate(gr.batch_effective_counts())]
    assert [len(k) for k in kept][:2] == [0, 1] and all(0 < len(kept[f]) < n for f, n in list(enumerate(gr.batch_effective_counts()))[2:5])
    # one image per frame matters: every frame with keypoints keeps a different set under its neighbour's image
    for f in (2, 3, 4):
        n = gr.batch_effective_counts()[f]
        assert _bits(gr.depth_gate(kps[f, :n], depth[f - 1])) != _bits(kept[f])


# ------------------------------------------------------------------------------------------------ distance filter
def test_match_scenes(oracle):
    seen = set()
    for n in gr.N256:
        idx, dist = gr.match_scene(n)
        seen |= set(dist.tolist())
        for maxd in gr.MATCH_MAXD:
            assert _bits(oracle.filter_matches(idx, dist, maxd)) == _bits(gr.filter_matches(idx, dist, maxd)), (n, maxd)
        for pattern in gr.PATTERNS:
            pi, pd = gr.match_scene(n, pattern)
            ref = gr.filter_matches(pi, pd, 50.0)
            assert ref[:, 0].tolist() == np.nonzero(gr.pattern_mask(n, pattern))[0].tolist()
            assert _bits(oracle.filter_matches(pi, pd, 50.0)) == _bits(ref)
    assert set(gr.MATCH_EDGE_DISTANCES) == {0, 49, 50, 51, 256, -1} <= seen
    idx, dist = gr.match_scene(513)
    kept = {maxd: set(dist[gr.filter_matches(idx, dist, maxd)[:, 0]].tolist()) for maxd in gr.MATCH_MAXD}
    assert 49 in kept[50.0] and 50 not in kept[50.0] and 49 in kept[49.5] and 50 not in kept[49.5]
    assert kept[0.0] == {-1} and kept[-1.0] == set() and 256 in kept[257.0] and kept[1e9] == set(dist.tolist())
    assert gr.filter_matches(idx[:0], dist[:0]).shape == (0, 3)


# ------------------------------------------------------------------------------------------------ back-projection, payload
def test_backproject_matches_oracle_and_scene_has_edges(oracle):
    fx, fy, cx, cy = gr.INTRINSICS
    for n in gr.N256:
        kps, desc, depth, classes = gr.edge_scene(n)
        w, oi = gr.backproject(kps, depth, fx, fy, cx, cy, gr.R_GENERAL, gr.T_GENERAL)
        w2, oi2 = oracle.backproject(kps, depth, fx, fy, cx, cy, gr.R_GENERAL, gr.T_GENERAL)
        assert _bits(oi) == _bits(oi2) and _bits(w) == _bits(w2), n
        assert (n == 0 and len(oi) == 0) or (0 < len(oi) and (n == 1 or len(oi) < n))
    a, b = classes["planted"]
    kept = [d for d, i in zip(gr.PLANTED_DEPTHS, range(a, b)) if i in set(oi.tolist())]
    assert kept == [300, 301, 2999, 999, 1000, 1001]       # 0.3 < (double)Z < 3.0: 300 * 0.001f = 0.3f lies ABOVE the double 0.3 ...
    assert float(F32(300) * F32(0.001)) > 0.3 and float(F32(3000) * F32(0.001)) > 3.0 > float(F32(2999) * F32(0.001))   # ... and 3000 above 3.0


def test_no_depth_separates_the_two_passes_of_publish_keyframe():
    """k_publish_keyframe evaluates (double)Z < 3.0 twice (count, then write).  No uint16 depth gives Z == 3.0f exactly — 3000 gives
    3.0000002f, 2999 gives 2.999f — so `<` and `<=` select the same keypoints at every depth; likewise Z == 0.3 never happens in
    double (float32(300 * 0.001f) > 0.3)."""
    z = np.arange(65536, dtype=np.uint16).astype(F32) * F32(0.001)
    assert not (z == F32(3.0)).any() and not (z.astype(np.float64) == 0.3).any()
    assert z[3000] == np.nextafter(F32(3.0), F32(4.0)) and z[2999] < F32(3.0)


FRAME_IDS = ["", "a", "ab", "abc", "abcd", "abcde", "abcdef", "abcdefg", "f" * 63]


def test_keyframe_payload_matches_oracle(oracle):
    fx, fy, cx, cy = gr.INTRINSICS
    q = (0.0, 0.0, np.sqrt(0.5), np.sqrt(0.5))
    kps, desc, depth, _ = gr.edge_scene(257)
    for fid in FRAME_IDS:
        want, m = gr.keyframe_payload(kps, desc, depth, fx, fy, cx, cy, gr.R_GENERAL, gr.T_GENERAL, (12, 345678), fid, 77, q)
        got, m2 = oracle.publish_keyframe(kps, desc, depth, fx, fy, cx, cy, gr.R_GENERAL, gr.T_GENERAL, (12, 345678), fid, 77, q)
        assert m == m2 and got == want, fid
    assert [len(f) for f in FRAME_IDS] == [0, 1, 2, 3, 4, 5, 6, 7, 63]
    for n in gr.N256:
        kps, desc, depth, _ = gr.edge_scene(n)
        want, m = gr.keyframe_payload(kps, desc, depth, fx, fy, cx, cy, gr.R_GENERAL, gr.T_GENERAL)
        got, m2 = oracle.publish_keyframe(kps, desc, depth, fx, fy, cx, cy, gr.R_GENERAL, gr.T_GENERAL)
        assert m == m2 and got == want, n
    assert gr.keyframe_payload(*gr.edge_scene(1)[:3], fx, fy, cx, cy, gr.R_GENERAL, gr.T_GENERAL)[1] == 1       # m = 1: no trailing pad
    k0, d0, z0, _ = gr.edge_scene(257)
    assert gr.keyframe_payload(k0, d0, np.zeros_like(z0), fx, fy, cx, cy, gr.R_GENERAL, gr.T_GENERAL)[1] == 0  # m = 0 with n > 0


# ------------------------------------------------------------------------------------------------ gray
def test_gray_matches_oracle(oracle):
    for variant in (0, 1):
        cb, cg, cr, shift = gr.GRAY_COEFFS[variant]
        assert cb + cg + cr == 1 << shift
        for rows in gr.GRAY_ROWS:
            for cols in gr.GRAY_COLS:
                bgr = gr.gray_scene(rows, cols, 3)
                for f in range(3):
                    assert _bits(gr.gray(bgr[f], variant)) == _bits(oracle.bgr_to_gray(bgr[f], variant)), (variant, rows, cols)
    bgr = gr.gray_scene(4, 7, 3)
    assert [tuple(p) for p in bgr[0].reshape(-1, 3)[:8].tolist()] == gr.GRAY_CORNERS and len(set(gr.GRAY_CORNERS)) == 8
    assert _bits(bgr[0]) != _bits(bgr[1]) != _bits(bgr[2])
    assert gr.gray(np.array([[[255, 255, 255], [0, 0, 0], [255, 0, 0], [0, 255, 0], [0, 0, 255]]], np.uint8)).tolist() == [[255, 0, 29, 150, 76]]


# ------------------------------------------------------------------------------------------------ Harris
def test_harris_matches_oracle(oracle):
    img, xs, ys = gr.harris_scene()
    assert img.shape == (20, 24) and xs.min() == ys.min() == -9 and xs.max() == 24 + 9 and ys.max() == 20 + 9
    assert {(x, y) for x in range(24) for y in range(20)} <= set(zip(xs.tolist(), ys.tolist()))
    for bs in gr.HARRIS_BLOCKS:
        ref = gr.harris_reference(bs)
        assert _bits(ref) == _bits(oracle.harris_responses(img, xs, ys, bs)), bs
        inside = (xs >= 0) & (ys >= 0) & (xs < 24) & (ys < 20)
        assert (ref[~inside] == 0).all() and (ref != 0).sum() == (24 - bs - 1) * (20 - bs - 1), bs   # every defined window responds


# ------------------------------------------------------------------------------------------------ association
def test_association_exact_scene(oracle):
    s = gr.assoc_exact_scene()
    obs, lm = s["obs"], s["lm"]
    args = (s["obs_desc"], s["obs_px"], s["lm_desc"], s["lm_xyz"], s["R"], s["t"]) + s["K"]
    ham = gr.hamming(s["obs_desc"], s["lm_desc"])
    assert [int(ham[obs[f"ham{h}"], lm[f"ham{h}"]]) for h in gr.ASSOC_HAMMING] == [0, 49, 50, 51, 256]
    off = ham.copy()
    for name, i in obs.items():                                  # nothing but the planted pairs is near any gate below 100
        for lname, j in lm.items():
            if lname.split("_")[0] == name.split("_")[0]:
                off[i, j] = 999
    assert off.min() > 60
    err = gr.reprojection_errors(s["obs_px"], s["lm_xyz"], s["R"], s["t"], *s["K"])
    assert err[obs["axis"], lm["axis"]] == 5.0
    assert err[obs["tie"], lm["tie_a"]] == err[obs["tie"], lm["tie_b"]] == err[obs["tie"], lm["tie_c"]] == 2.0 and lm["tie_a"] < lm["tie_b"] < lm["tie_c"]
    assert [err[obs["later"], lm[k]] for k in ("later_far", "later_near", "later_mid")] == [3.0, 1.0, 2.0] and lm["later_far"] < lm["later_near"] < lm["later_mid"]
    assert s["lm_xyz"][lm["behind"], 2] < 0 and s["lm_xyz"][lm["plane"], 2] == 0
    assert err[obs["behind_hit"], lm["behind"]] == err[obs["plane_hit"], lm["plane"]] == 2.5 and err[obs["plane_miss"], lm["plane"]] > 5
    assert np.isfinite(s["obs_px"]).all() and np.isfinite(s["lm_xyz"]).all()
    taken = {}
    for md in gr.ASSOC_MAX_DESC:
        best, offs, cand = gr.assoc_reference("exact", max_desc=md)
        assert _bits(best) == _bits(oracle.associate(*args, max_desc=md)), md
        taken[md] = [h for h in gr.ASSOC_HAMMING if best[obs[f"ham{h}"]] >= 0]
        assert all(best[obs[f"ham{h}"]] in (-1, lm[f"ham{h}"]) for h in gr.ASSOC_HAMMING)
        assert offs[-1] == len(cand) and (np.diff(offs) >= 0).all()
        for i in range(len(best)):
            c = cand[offs[i]:offs[i + 1]]
            assert (np.diff(c) > 0).all() and set(c.tolist()) == set(np.nonzero(ham[i] < min(np.ceil(md), 257))[0].tolist())
    assert taken == {50.0: [0, 49], 49.5: [0, 49], 50.5: [0, 49, 50], 0.0: [], 0.5: [0], 256.0: [0, 49, 50, 51], 257.0: [0, 49, 50, 51, 256],
                     1000.0: [0, 49, 50, 51, 256]}
    best = gr.assoc_reference("exact")[0]
    assert best[obs["ham49"]] == lm["ham49"] and best[obs["tie"]] == lm["tie_a"] and best[obs["later"]] == lm["later_near"]
    assert best[obs["behind_hit"]] == lm["behind"] and best[obs["plane_hit"]] == lm["plane"]
    assert best[obs["behind_miss"]] == -1 and best[obs["plane_miss"]] == -1
    assert best[obs["axis"]] == -1                                            # refused at exactly 5.0 ...
    up = np.nextafter(5.0, np.inf)
    b2 = gr.assoc_reference("exact", max_reproj=up)[0]
    assert b2[obs["axis"]] == lm["axis"] and _bits(b2) == _bits(oracle.associate(*args, max_reproj=up))   # ... and taken just above


def test_association_sweep_scenes(oracle):
    assert {a for a, _ in gr.ASSOC_SIZES} == {1, 3, 4, 5, 1023, 1024, 1025, 2049} and {b for _, b in gr.ASSOC_SIZES} == {1, 63, 64, 65, 129}
    gates = set()
    for nobs, nlm in gr.ASSOC_SIZES:
        s = gr.assoc_sweep_scene(nobs, nlm)
        best, offs, cand = gr.assoc_reference("sweep", nobs, nlm)
        assert len(best) == nobs and len(s["lm_desc"]) == nlm
        assert _bits(best) == _bits(oracle.associate(s["obs_desc"], s["obs_px"], s["lm_desc"], s["lm_xyz"], s["R"], s["t"], *s["K"])), (nobs, nlm)
        assert np.isfinite(s["obs_px"]).all() and np.isfinite(s["lm_xyz"]).all()
        if nobs >= 1023 and nlm >= 64:
            ham = gr.hamming(s["obs_desc"], s["lm_desc"]); gates |= set(np.unique(ham[(ham >= 48) & (ham <= 52)]).tolist())
            assert (best >= 0).sum() > 50 and (best < 0).sum() > 50 and 0 < len(cand) < nobs * nlm
            behind = np.nonzero(s["lm_xyz"][:, 2] < 0)[0]
            assert np.isin(best, behind).any() and np.isin(cand, behind).any()       # (-1, -1) projections that do get associated
    assert gates == {48, 49, 50, 51, 52}
