"""numpy statements of what include/dvslam_hip.h promises for the glue either side of the hot path (csrc/frontend.hip), written from
the header text and the kernel comments — not from oracle/frontend_oracle.cpp — plus the scenes that put every gate, rounding rule and
trip edge of those kernels under a keypoint.  tests/test_glue_ref_cpu.py checks the statements against the oracle and the scenes'
preconditions; tests/test_gpu_glue_edges.py compares the HIP entry points with them bit for bit.
Float32 steps are separate numpy float32 operations (the library is built with -ffp-contract=off: nothing is fused)."""
import functools
import struct
import numpy as np
from dvslam_amd._lib import KP_DTYPE

F32 = np.float32
N256 = (0, 1, 255, 256, 257, 513)                       # compactions that walk 256 elements per trip
N1024 = N256 + (1023, 1024, 1025, 2049)                 # k_filter_depth: 1024 per trip as four chunks of 256


def f32(v):
    return np.asarray(v, F32)


# ------------------------------------------------------------------------------------------------ the operations
def round_px(v):
    """std::round on a float32 (half away from zero), exact: the float64 sum v + copysign(0.5, v) of a float32 is not rounded"""
    v = f32(v).astype(np.float64)
    return np.trunc(v + np.copysign(0.5, v)).astype(np.int64)


GRAY_COEFFS = {0: (3735, 19235, 9798, 15), 1: (1868, 9617, 4899, 14)}


def gray(bgr, variant=0):
    cb, cg, cr, shift = GRAY_COEFFS[variant]
    p = np.asarray(bgr).astype(np.int64)
    return ((p[..., 0] * cb + p[..., 1] * cg + p[..., 2] * cr + (1 << (shift - 1))) >> shift).astype(np.uint8)


def _depth_at(kps, depth):
    """(inside, float32 metres) under every keypoint's rounded pixel; outside the image: not inside, 0"""
    rows, cols = depth.shape
    x = round_px(kps["x"]); y = round_px(kps["y"])
    inside = (x >= 0) & (y >= 0) & (x < cols) & (y < rows)
    d = np.asarray(depth)[np.where(inside, y, 0), np.where(inside, x, 0)]
    z = d.astype(F32) * F32(0.001)
    return inside, np.where(inside, z, F32(0)).astype(F32)


def gate_verdict(depth_u16, dmin=0.3, dmax=3.0):
    """the depth gate on raw depth values: keep not (z < dmin or z > dmax)"""
    z = np.asarray(depth_u16).astype(F32) * F32(0.001)
    return ~((z < F32(dmin)) | (z > F32(dmax)))


def depth_gate(kps, depth, dmin=0.3, dmax=3.0):
    """indices of the keypoints dvs_filter_depth* keep, in order"""
    inside, z = _depth_at(kps, depth)
    keep = inside & ~((z < F32(dmin)) | (z > F32(dmax)))
    return np.nonzero(keep)[0].astype(np.int32)


def filter_matches(idx, dist, maxd=50.0):
    idx = np.asarray(idx, np.int32); dist = np.asarray(dist, np.int32)
    keep = np.nonzero(dist.astype(F32) < F32(maxd))[0]
    return np.stack([keep.astype(np.int32), idx[keep], dist[keep]], axis=1).astype(np.int32).reshape(-1, 3)


def backproject(kps, depth, fx, fy, cx, cy, R, t):
    """-> (world float64 (m, 3), keypoint indices int32 (m,))"""
    fx, fy, cx, cy = F32(fx), F32(fy), F32(cx), F32(cy)
    R = np.asarray(R, np.float64).reshape(3, 3); t = np.asarray(t, np.float64).reshape(3)
    _, z = _depth_at(kps, depth)
    px = f32(kps["x"]); py = f32(kps["y"])
    X = ((px - cx) * z) / fx
    Y = ((py - cy) * z) / fy
    z64 = z.astype(np.float64)
    keep = (z64 > 0.3) & (z64 < 3.0)
    v0, v1, v2 = X.astype(np.float64)[keep], Y.astype(np.float64)[keep], z64[keep]
    world = np.stack([(R[r, 0] * v0 + R[r, 1] * v1 + R[r, 2] * v2) + t[r] for r in range(3)], axis=1).reshape(-1, 3)
    return world, np.nonzero(keep)[0].astype(np.int32)


def hand_cdr(stamp, frame_id, kf_id, trans, rot, landmarks, observations):
    """Keyframe.msg straight from the CDR rules: align every primitive to its size relative to the byte after the 4-byte
    encapsulation header."""
    b = bytearray()

    def put(fmt, v):
        size = struct.calcsize(fmt)
        while len(b) % size:
            b.append(0)
        b.extend(struct.pack("<" + fmt, v))

    put("i", stamp[0]); put("I", stamp[1])
    put("I", len(frame_id) + 1); b.extend(frame_id.encode() + b"\0")
    put("Q", kf_id)
    for v in trans: put("d", v)
    for v in rot: put("d", v)
    put("I", len(landmarks))
    for lid, x, y, z in landmarks:
        put("Q", lid); put("d", x); put("d", y); put("d", z)
    put("I", len(observations))
    for lid, u, v, d in observations:
        put("Q", lid); put("d", u); put("d", v); put("I", len(d)); b.extend(bytes(d))
    return bytes([0, 1, 0, 0]) + bytes(b)


def keyframe_payload(kps, desc, depth, fx, fy, cx, cy, R, t, stamp=(0, 0), frame_id="camera_link", keyframe_id=0,
                     q_xyzw=(0.0, 0.0, 0.0, 1.0), trans=None):
    """-> (payload bytes, landmarks): landmark_id = keypoint index, float64 pixels, 32-byte descriptors"""
    world, oi = backproject(kps, depth, fx, fy, cx, cy, R, t)
    desc = np.asarray(desc, np.uint8).reshape(-1, 32)
    lms = [(int(i), float(w[0]), float(w[1]), float(w[2])) for i, w in zip(oi, world)]
    obs = [(int(i), float(kps["x"][i]), float(kps["y"][i]), desc[i]) for i in oi]
    return hand_cdr(stamp, frame_id, keyframe_id, t if trans is None else trans, q_xyzw, lms, obs), len(oi)


_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def hamming(a, b):
    """(na, nb) Hamming distances of 32-byte rows"""
    a = np.asarray(a, np.uint8).reshape(-1, 32); b = np.asarray(b, np.uint8).reshape(-1, 32)
    return _POP[a[:, None, :] ^ b[None, :, :]].sum(axis=2)


def reprojection_errors(obs_px, lm_xyz, R, t, fx, fy, cx, cy):
    """(nobs, nlm) float64: |pixel - project(R^T (l - t))|, a landmark that is not in front of the camera projecting to (-1, -1)"""
    R = np.asarray(R, np.float64).reshape(3, 3); t = np.asarray(t, np.float64).reshape(3)
    l = f32(lm_xyz).reshape(-1, 3).astype(np.float64); o = f32(obs_px).reshape(-1, 2)
    d0, d1, d2 = l[:, 0] - t[0], l[:, 1] - t[1], l[:, 2] - t[2]
    c0 = R[0, 0] * d0 + R[1, 0] * d1 + R[2, 0] * d2
    c1 = R[0, 1] * d0 + R[1, 1] * d1 + R[2, 1] * d2
    c2 = R[0, 2] * d0 + R[1, 2] * d1 + R[2, 2] * d2
    front = ~(c2 <= 0)
    den = np.where(front, c2, 1.0)
    u = np.where(front, (fx * c0 / den + cx).astype(F32), F32(-1)).astype(F32)
    v = np.where(front, (fy * c1 / den + cy).astype(F32), F32(-1)).astype(F32)
    dx = (o[:, 0][:, None] - u[None, :]).astype(np.float64); dy = (o[:, 1][:, None] - v[None, :]).astype(np.float64)
    return np.sqrt(dx * dx + dy * dy)


def associate(obs_desc, obs_px, lm_desc, lm_xyz, R, t, fx, fy, cx, cy, max_desc=50.0, max_reproj=5.0):
    """-> (best int32 (nobs,), candidate offsets int64 (nobs + 1,), candidate landmarks int32): candidate iff Hamming < ceil(max_desc)
    (capped at 257), in landmark order; best = the first candidate with the smallest error < max_reproj, else -1"""
    nobs = len(np.asarray(obs_desc).reshape(-1, 32)); nlm = len(np.asarray(lm_desc).reshape(-1, 32))
    if nobs == 0 or nlm == 0:
        return np.full(nobs, -1, np.int32), np.zeros(nobs + 1, np.int64), np.zeros(0, np.int32)
    cand = hamming(obs_desc, lm_desc) < min(int(np.ceil(max_desc)), 257)
    err = reprojection_errors(obs_px, lm_xyz, R, t, fx, fy, cx, cy)
    e = np.where(cand & (err < max_reproj), err, np.inf)
    j = np.argmin(e, axis=1)                                     # first occurrence of the minimum
    best = np.where(np.isfinite(e[np.arange(nobs), j]), j, -1).astype(np.int32)
    offs = np.concatenate([[0], np.cumsum(cand.sum(axis=1))]).astype(np.int64)
    return best, offs, np.nonzero(cand)[1].astype(np.int32)


def harris(img, xs, ys, bs=7, k=F32(0.04)):
    """whole-image integer gradient maps, box sums, the float32 expression in the source's order; 0 where the window (and its
    gradients' neighbours) would leave the image"""
    I = np.asarray(img).astype(np.int64)
    Ix = np.zeros_like(I); Iy = np.zeros_like(I)
    Ix[1:-1, 1:-1] = (I[1:-1, 2:] - I[1:-1, :-2]) * 2 + (I[:-2, 2:] - I[:-2, :-2]) + (I[2:, 2:] - I[2:, :-2])
    Iy[1:-1, 1:-1] = (I[2:, 1:-1] - I[:-2, 1:-1]) * 2 + (I[2:, :-2] - I[:-2, :-2]) + (I[2:, 2:] - I[:-2, 2:])
    r = bs // 2
    out = np.zeros(len(xs), F32)
    scale = F32(1.0) / (F32(4 * bs) * F32(255.0))
    s4 = scale * scale * scale * scale
    k = F32(k)
    for i, (x, y) in enumerate(zip(xs, ys)):
        if not (x - r - 1 >= 0 and y - r - 1 >= 0 and x - r + bs <= I.shape[1] - 1 and y - r + bs <= I.shape[0] - 1):
            continue
        wx = Ix[y - r:y - r + bs, x - r:x - r + bs]; wy = Iy[y - r:y - r + bs, x - r:x - r + bs]
        a = F32(int((wx * wx).sum())); b = F32(int((wy * wy).sum())); c = F32(int((wx * wy).sum()))
        s = a + b
        out[i] = (a * b - c * c - (k * s) * s) * s4
    return out


# ------------------------------------------------------------------------------------------------ scenes
ROWS, COLS = 24, 40                                       # the depth image of every depth scene
PLANTED_DEPTHS = (0, 299, 300, 301, 2999, 3000, 3001, 65535, 999, 1000, 1001)
PLANT_ROW = 20                                            # planted depth p sits at (x = 2 + p's position, y = PLANT_ROW)
KEEP_PX, DROP_PX = (2, 2), (3, 2)                         # (x, y) of a pixel the default gate keeps / drops
GATES = {"default": (0.3, 3.0), "point": (1.0, 1.0), "empty": (2.0, 1.0)}
INTRINSICS = (615.5, 616.25, 320.1, 241.3)                # not representable in float32 after the arithmetic
R_GENERAL = np.array([[0.9975, -0.0499, 0.05], [0.0524, 0.9974, -0.0498], [-0.0474, 0.0523, 0.9975]])
T_GENERAL = np.array([0.1, -0.2, 0.05])


def nextafter0(v):
    return np.nextafter(F32(v), F32(0))


def depth_image(shift=0):
    """checkerboard of a kept (1500) and a dropped (0) depth — the two pixels either side of EVERY half-way coordinate get different
    verdicts, in x and in y — with the planted depths in row PLANT_ROW; `shift` moves the checkerboard by one pixel per unit"""
    yy, xx = np.mgrid[0:ROWS, 0:COLS]
    d = np.where((xx + yy + shift) % 2 == 0, 1500, 0).astype(np.uint16)
    for i, v in enumerate(PLANTED_DEPTHS):
        d[PLANT_ROW, 2 + i] = v
    return d


def rounding_values(size):
    """coordinates on the rounding rule and on the image border, for an axis of `size` pixels"""
    return [F32(10.5), nextafter0(10.5), F32(11.5), nextafter0(11.5), F32(0.49999997), F32(-0.4), F32(-0.5), F32(size - 0.5),
            nextafter0(size - 0.5), F32(1e5)]


def edge_keypoints():
    """keypoints on every planted depth, and the rounding set on x (rows 4 and 5) and on y (columns 6 and 7)
    -> (kps, classes): classes names the index ranges"""
    pts, classes = [], {}

    def add(name, ps):
        classes[name] = (len(pts), len(pts) + len(ps)); pts.extend(ps)

    add("planted", [(F32(2 + i), F32(PLANT_ROW)) for i in range(len(PLANTED_DEPTHS))])
    add("round_x", [(v, F32(y)) for v in rounding_values(COLS) for y in (4, 5)])
    add("round_y", [(F32(x), v) for v in rounding_values(ROWS) for x in (6, 7)])
    kps = np.zeros(len(pts), KP_DTYPE)
    kps["x"] = [p[0] for p in pts]; kps["y"] = [p[1] for p in pts]
    return kps, classes


def _dress(kps, seed):
    """every keypoint distinguishable, so a compaction that moves the wrong row shows"""
    rng = np.random.default_rng(seed); n = len(kps)
    kps["size"] = rng.uniform(20, 40, n).astype(F32); kps["angle"] = rng.uniform(0, 360, n).astype(F32)
    kps["response"] = np.arange(n, dtype=F32) + F32(7); kps["octave"] = rng.integers(0, 8, n); kps["class_id"] = -1
    return kps


def descriptors(n, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, 32), dtype=np.uint8)


PATTERNS = ("all", "none", "alternating", "last", "chunk_first")


def pattern_mask(n, pattern):
    i = np.arange(n)
    return {"all": i >= 0, "none": i < 0, "alternating": i % 2 == 1, "last": i == n - 1, "chunk_first": i % 256 == 0}[pattern]


@functools.lru_cache(maxsize=None)
def pattern_scene(n, pattern):
    """n keypoints whose verdict under the default gate follows `pattern` (sub-pixel offsets that do not change the rounded pixel)
    -> (kps, desc, depth, mask)"""
    rng = np.random.default_rng(1000 + n)
    mask = pattern_mask(n, pattern)
    kps = np.zeros(n, KP_DTYPE)
    kps["x"] = (np.where(mask, KEEP_PX[0], DROP_PX[0]) + rng.uniform(-0.45, 0.45, n)).astype(F32)
    kps["y"] = (KEEP_PX[1] + rng.uniform(-0.45, 0.45, n)).astype(F32)
    return _dress(kps, n), descriptors(n, 2000 + n), depth_image(), mask


@functools.lru_cache(maxsize=None)
def edge_scene(n=1025, seed=0):
    """the edge keypoints first (a kept one in front, so n = 1 keeps something), random ones over and around the image behind them
    -> (kps, desc, depth, classes)"""
    ek, classes = edge_keypoints()
    rng = np.random.default_rng(seed)
    kps = np.zeros(max(n, len(ek) + 1), KP_DTYPE)
    kps["x"] = rng.uniform(-2, COLS + 1, len(kps)).astype(F32); kps["y"] = rng.uniform(-2, ROWS + 1, len(kps)).astype(F32)
    kps["x"][0], kps["y"][0] = KEEP_PX
    kps[1:1 + len(ek)] = ek
    classes = {k: (a + 1, b + 1) for k, (a, b) in classes.items()}
    kps = _dress(kps, seed + 1)[:n]
    return kps, descriptors(n, seed + 2), depth_image(), classes


def padded(img, pad_bytes, fill=0xEE):
    """the same image as a view into rows `pad_bytes` wider"""
    rows, cols = img.shape
    step = cols * img.itemsize + pad_bytes
    buf = np.full(rows * step, fill, np.uint8)
    view = np.ndarray((rows, cols), img.dtype, buf, 0, (step, img.itemsize))
    view[:] = img
    return view


BATCH_COUNTS = (0, 1, 257, 300, 309, -3)                  # the last two are clamped to the stride and to 0
BATCH_STRIDE = 300


@functools.lru_cache(maxsize=None)
def batch_scene():
    """six frames of BATCH_STRIDE keypoint rows, one depth image per frame (the checkerboard shifted by the frame number)"""
    F = len(BATCH_COUNTS)
    kps = np.zeros((F, BATCH_STRIDE), KP_DTYPE)
    for f in range(F):
        kps[f] = edge_scene(BATCH_STRIDE, 40 + f)[0]
        kps[f, 0]["x"] = KEEP_PX[0] + f % 2                 # kept under this frame's checkerboard, so d_n = 1 keeps its keypoint
    kps = _dress(kps.reshape(-1), 50).reshape(F, BATCH_STRIDE)
    depth = np.stack([depth_image(f) for f in range(F)])
    return kps, descriptors(F * BATCH_STRIDE, 51).reshape(F, BATCH_STRIDE, 32), depth, np.array(BATCH_COUNTS, np.int32)


def batch_effective_counts():
    return [min(max(n, 0), BATCH_STRIDE) for n in BATCH_COUNTS]


MATCH_EDGE_DISTANCES = (49, 50, 0, 51, 256, -1)
MATCH_MAXD = (50.0, 49.5, 0.0, -1.0, 257.0, 1e9)


@functools.lru_cache(maxsize=None)
def match_scene(n, pattern="edges"):
    """-> (train_idx, dist): the edge distances first, random ones behind; or a keep pattern under max_distance 50 (49 kept, 50 not)"""
    rng = np.random.default_rng(300 + n)
    idx = rng.integers(0, 2000, n).astype(np.int32)
    if pattern == "edges":
        dist = rng.integers(0, 120, n).astype(np.int32)
        dist[:len(MATCH_EDGE_DISTANCES)] = MATCH_EDGE_DISTANCES[:n]
        if n > 1: dist[-1] = 49
    else:
        dist = np.where(pattern_mask(n, pattern), 49, 50).astype(np.int32)
    return idx, dist


GRAY_COLS = (1, 2, 3, 4, 5, 7, 255, 256, 257, 259)
GRAY_ROWS = (1, 3, 4, 5)
GRAY_CORNERS = [(b, g, r) for b in (0, 255) for g in (0, 255) for r in (0, 255)]   # each channel alone 0 or 255


@functools.lru_cache(maxsize=None)
def gray_scene(rows, cols, nimg=1):
    """random colours with the eight corner colours in front of every image (as many as fit) -> uint8 (nimg, rows, cols, 3)"""
    rng = np.random.default_rng(rows * 1000 + cols)
    bgr = rng.integers(0, 256, (nimg, rows, cols, 3), dtype=np.uint8)
    flat = bgr.reshape(nimg, rows * cols, 3)
    for f in range(nimg):
        k = min(len(GRAY_CORNERS), rows * cols)
        flat[f, :k] = np.roll(np.array(GRAY_CORNERS, np.uint8), f, axis=0)[:k]
    return bgr


HARRIS_ROWS, HARRIS_COLS = 20, 24
HARRIS_BLOCKS = tuple(range(1, 9))


@functools.lru_cache(maxsize=None)
def harris_scene():
    """-> (img, xs, ys): every pixel is a query point, and so is every position up to 9 pixels outside the image on every side"""
    img = np.random.default_rng(77).integers(0, 256, (HARRIS_ROWS, HARRIS_COLS), dtype=np.uint8)
    ys, xs = np.mgrid[-9:HARRIS_ROWS + 10, -9:HARRIS_COLS + 10]
    return img, xs.reshape(-1).astype(np.int32), ys.reshape(-1).astype(np.int32)


@functools.lru_cache(maxsize=None)
def harris_reference(bs):
    img, xs, ys = harris_scene()
    return harris(img, xs, ys, bs)


# association: R = I, t = 0, fx = fy = 512: a landmark (du / 256, dv / 256, 2) projects to (cx + du, cy + dv) EXACTLY
ASSOC_K = (512.0, 512.0, 320.0, 240.0)
ASSOC_HAMMING = (0, 49, 50, 51, 256)
ASSOC_MAX_DESC = (50.0, 49.5, 50.5, 0.0, 0.5, 256.0, 257.0, 1000.0)


def flip_bits(desc, k, rng):
    d = desc.copy()
    for b in rng.choice(256, k, replace=False):
        d[b // 8] ^= np.uint8(1 << (b % 8))
    return d


@functools.lru_cache(maxsize=None)
def assoc_exact_scene():
    """planted pairs; every observation has a descriptor of its own (random 256-bit rows lie ~128 bits apart), so only the planted
    landmarks are its candidates under the default gate -> dict with the arrays and `obs` / `lm`: name -> index"""
    rng = np.random.default_rng(9)
    fx, fy, cx, cy = ASSOC_K
    obs_d, obs_p, lm_d, lm_x, obs, lm = [], [], [], [], {}, {}

    def add_obs(name, desc, u, v):
        obs[name] = len(obs_d); obs_d.append(desc); obs_p.append((u, v))

    def add_lm(name, desc, du, dv, z=2.0):
        lm[name] = len(lm_d); lm_d.append(desc); lm_x.append((du / 256.0, dv / 256.0, z))

    def fresh():
        return rng.integers(0, 256, 32, dtype=np.uint8)

    for k, h in enumerate(ASSOC_HAMMING):                    # the Hamming gate: one pixel of reprojection error, h flipped bits
        d = fresh()
        add_obs(f"ham{h}", d, cx + 10 + 20 * k + 1, cy - 20); add_lm(f"ham{h}", flip_bits(d, h, rng), 10 + 20 * k, -20)
    d = fresh()                                              # the reprojection gate: on the optical axis, error exactly 5
    add_obs("axis", d, cx + 3, cy + 4); add_lm("axis", d, 0, 0)
    d = fresh()                                              # equal errors: the first in landmark order wins
    add_obs("tie", d, cx + 50, cy + 30); add_lm("tie_a", d, 48, 30); add_lm("tie_b", d, 52, 30); add_lm("tie_c", d, 50, 32)
    d = fresh()                                              # a later candidate with a strictly smaller error wins
    add_obs("later", d, cx - 60, cy + 7); add_lm("later_far", d, -63, 7); add_lm("later_near", d, -61, 7); add_lm("later_mid", d, -58, 7)
    for name, z in (("behind", -1.0), ("plane", 0.0)):       # c2 < 0 and c2 == 0: projection (-1, -1)
        d = fresh()
        add_obs(name + "_hit", d, 0.5, 1.0); add_obs(name + "_miss", d, cx, cy); add_lm(name, d, 5, 5, z)
    return dict(obs_desc=np.array(obs_d, np.uint8), obs_px=np.array(obs_p, F32), lm_desc=np.array(lm_d, np.uint8),
                lm_xyz=np.array(lm_x, F32), R=np.eye(3), t=np.zeros(3), K=ASSOC_K, obs=obs, lm=lm)


ASSOC_SIZES = ((1, 1), (3, 63), (4, 64), (5, 65), (1023, 129), (1024, 64), (1025, 65), (2049, 129), (2049, 1))


@functools.lru_cache(maxsize=None)
def assoc_sweep_scene(nobs, nlm):
    """a general pose; most observations re-observe a landmark with 40 .. 60 flipped bits (either side of the Hamming gate) and a few
    pixels of noise (either side of the reprojection gate); every fourth landmark lies behind the camera; duplicates in the database"""
    rng = np.random.default_rng(nobs * 131 + nlm)
    R, t = R_GENERAL, T_GENERAL
    fx, fy, cx, cy = 600.0, 601.5, 320.25, 240.75
    lm_desc = descriptors(nlm, nobs + 7 * nlm)
    lm_xyz = np.stack([rng.uniform(-2, 2, nlm), rng.uniform(-1.5, 1.5, nlm), rng.uniform(2, 6, nlm)], axis=1).astype(F32)
    lm_xyz[3::4, 2] *= -1
    if nlm > 10:
        lm_desc[7] = lm_desc[3]; lm_xyz[7] = lm_xyz[3]
    obs_desc = descriptors(nobs, nobs + 11 * nlm)
    obs_px = rng.uniform(0, 640, (nobs, 2)).astype(F32)
    for i in range(nobs):
        if i % 8 == 7:
            continue                                          # unrelated observation
        j = int(rng.integers(0, nlm))
        obs_desc[i] = flip_bits(lm_desc[j], int(rng.integers(40, 61)), rng)
        pc = R.T @ (lm_xyz[j].astype(np.float64) - t)
        if pc[2] > 0:
            obs_px[i] = [fx * pc[0] / pc[2] + cx + rng.normal(0, 3.0), fy * pc[1] / pc[2] + cy + rng.normal(0, 3.0)]
        else:
            obs_px[i] = [0.5 + rng.normal(0, 2.0), 1.0 + rng.normal(0, 2.0)]
    return dict(obs_desc=obs_desc, obs_px=obs_px, lm_desc=lm_desc, lm_xyz=lm_xyz, R=R, t=t, K=(fx, fy, cx, cy))


@functools.lru_cache(maxsize=None)
def assoc_reference(kind, nobs=0, nlm=0, max_desc=50.0, max_reproj=5.0):
    s = assoc_exact_scene() if kind == "exact" else assoc_sweep_scene(nobs, nlm)
    return associate(s["obs_desc"], s["obs_px"], s["lm_desc"], s["lm_xyz"], s["R"], s["t"], *s["K"], max_desc, max_reproj)
