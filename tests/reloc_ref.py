"""The relocalisation rule of include/dvslam_hip.h "Relocalisation", restated in numpy and plain Python: the reference of
tests/test_gpu_reloc.py.  Stages 1-3 are integers (compared bit for bit); stage 4 is dvs_solve_pnp_ransac's procedure, which the caller
passes in as a function (the GPU tests pass the product's own host call, the CPU tests the oracle's statement of it); the host conversion
of its record is restated here with math.sin / math.cos, every expression in the header's order; stage 5 is map_track_ref.track."""
import math
import numpy as np
import map_track_ref as mr

OK, FEW_PAIRS, NO_POSE, NOT_CONFIRMED = 0, 1, 2, 3
KP_DTYPE = mr.KP_DTYPE
LM_RECORD = np.dtype([("best_k", "<i4"), ("d_best", "<i4"), ("d_second", "<i4"), ("proposed", "<i4"), ("kept", "<i4")])
DEFAULTS = dict(max_hamming=50, ratio_pct=75, min_pairs=20, pnp_iterations=512, pnp_reproj_err=4.0, pnp_confidence=0.99, min_pnp_inliers=15,
                min_confirmed=30, seed=0)
# the largest |R - R_true|, |t - t_true| entry of locate() on scene() with the oracle's RANSAC on the CPU (tests/test_reloc_cpu.py measures
# it again); the device is held to ten times this
POSE_MEASURED = 8.0e-4          # measured 7.48e-04 (the translation; the rotation 1.03e-04): the scene's pixel noise, not arithmetic
_POP = np.array([bin(v).count("1") for v in range(256)], np.int32)


class Params:
    def __init__(self, K4, **kw):
        self.K4 = [float(v) for v in K4]
        for k, v in DEFAULTS.items():
            setattr(self, k, v)
        for k, v in kw.items():
            if k not in DEFAULTS:
                raise AttributeError(k)
            setattr(self, k, v)

    def with_(self, **kw):
        q = Params(self.K4)
        q.__dict__.update(self.__dict__)
        q.__dict__.update(kw)
        return q


def distances(ldesc, kdesc):
    """hamming(desc_j, desc_k) for every pair -> int32 (n_lm, n_kp)"""
    ldesc = np.asarray(ldesc, np.uint8).reshape(-1, 32); kdesc = np.asarray(kdesc, np.uint8).reshape(-1, 32)
    out = np.zeros((len(ldesc), len(kdesc)), np.int32)
    for j0 in range(0, len(ldesc), 256):
        out[j0:j0 + 256] = _POP[ldesc[j0:j0 + 256, None, :] ^ kdesc[None, :, :]].sum(2)
    return out


def finite_rows(xyz):
    return np.isfinite(np.asarray(xyz, np.float32).reshape(-1, 3)).all(1)


def search(P, xyz, ldesc, kdesc):
    """stage 1 -> LM_RECORD per landmark, kept still 0"""
    n_lm, n_kp = len(ldesc), len(kdesc)
    rec = np.zeros(n_lm, LM_RECORD)
    rec["best_k"] = rec["d_best"] = rec["d_second"] = -1
    if n_kp == 0 or n_lm == 0:
        return rec
    D = distances(ldesc, kdesc)
    fin = finite_rows(xyz)
    for j in range(n_lm):
        if not fin[j]:
            continue
        row = D[j]
        best = int(np.argmin(row))                              # the first smallest: the smallest (d, k)
        d_best = int(row[best])
        d_second = int(np.delete(row, best).min()) if n_kp > 1 else -1
        ratio_ok = d_second < 0 or P.ratio_pct <= 0 or d_best * 100 < P.ratio_pct * d_second
        rec[j] = (best, d_best, d_second, 1 if (d_best < P.max_hamming and ratio_ok) else 0, 0)
    return rec


def assign(rec, n_kp):
    """stage 2 -> (kp_lm int32 [n_kp] (-1: none), kp_dist int32 [n_kp] (-1: none)); sets rec["kept"]"""
    kp_lm = np.full(n_kp, -1, np.int32); kp_dist = np.full(n_kp, -1, np.int32)
    best = {}
    for j in range(len(rec)):
        if rec[j]["proposed"]:
            k, key = int(rec[j]["best_k"]), (int(rec[j]["d_best"]), j)
            if k not in best or key < best[k]:
                best[k] = key
    rec["kept"] = 0
    for k, (d, j) in best.items():
        kp_lm[k], kp_dist[k] = j, d
        rec[j]["kept"] = 1
    return kp_lm, kp_dist


def pair_list(xyz, kps, kp_lm, kp_dist):
    """stage 3 -> dict(lm_row, kp_index, dist int32 [m]; obj float32 (m, 3); img float32 (m, 2)) in ascending keypoint index"""
    ks = np.flatnonzero(kp_lm >= 0).astype(np.int32)
    rows = kp_lm[ks].astype(np.int32)
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    img = np.stack([kps["x"][ks], kps["y"][ks]], 1).astype(np.float32).reshape(-1, 2)
    return dict(lm_row=rows, kp_index=ks, dist=kp_dist[ks].astype(np.int32), obj=np.ascontiguousarray(xyz[rows]).reshape(-1, 3), img=np.ascontiguousarray(img))


def stages123(P, xyz, ldesc, kps, kdesc):
    rec = search(P, xyz, ldesc, kdesc)
    kp_lm, kp_dist = assign(rec, len(kps))
    out = pair_list(xyz, kps, kp_lm, kp_dist)
    out.update(rec=rec, n_proposed=int(rec["proposed"].sum()), n_pairs=len(out["lm_row"]))
    return out


def brute(P, xyz, ldesc, kdesc):
    """stages 1-2 a second time, with sets and loops and no shared helper -> (set of (landmark, keypoint, d) proposals, dict keypoint -> (landmark, d))"""
    proposals = set()
    for j in range(len(ldesc)):
        if not all(math.isfinite(float(v)) for v in xyz[j]):
            continue
        ds = [sum(bin(int(a) ^ int(b)).count("1") for a, b in zip(ldesc[j], kdesc[k])) for k in range(len(kdesc))]
        if not ds:
            continue
        order = sorted(range(len(ds)), key=lambda k: (ds[k], k))
        b = order[0]
        others = [ds[k] for k in order[1:]]
        if ds[b] >= P.max_hamming:
            continue
        if others and P.ratio_pct > 0 and not ds[b] * 100 < P.ratio_pct * min(others):
            continue
        proposals.add((j, b, ds[b]))
    kept = {}
    for k in {p[1] for p in proposals}:
        d, j = min((p[2], p[0]) for p in proposals if p[1] == k)
        kept[k] = (j, d)
    return proposals, kept


def rodrigues_pose(rvec, tvec):
    """stage 4's host conversion: (rvec, tvec) of x_cam = R_cw X + tvec -> camera-to-world (R 3x3, t 3), in the header's arithmetic"""
    w = [float(v) for v in rvec]; tv = [float(v) for v in tvec]
    th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
    th = math.sqrt(th2)
    K = [0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0]
    if th < 1e-12:
        Rcw = [(1.0 if k % 4 == 0 else 0.0) + K[k] for k in range(9)]
    else:
        A = math.sin(th) / th; B = (1.0 - math.cos(th)) / th2
        Rcw = [0.0] * 9
        for i in range(3):
            for j in range(3):
                k2 = (K[3 * i] * K[j] + K[3 * i + 1] * K[3 + j]) + K[3 * i + 2] * K[6 + j]
                Rcw[3 * i + j] = ((1.0 if i == j else 0.0) + A * K[3 * i + j]) + B * k2
    R = np.array([Rcw[3 * j + i] for i in range(3) for j in range(3)]).reshape(3, 3)
    t = np.array([-((Rcw[i] * tv[0] + Rcw[3 + i] * tv[1]) + Rcw[6 + i] * tv[2]) for i in range(3)])
    return R, t


def locate(P, MP, xyz, ldesc, kps, kdesc, pnp):
    """the whole rule.  MP: the map_track_ref.Params of the confirming handle; pnp(obj, img, K4, iterations, reproj_err, confidence, seed) ->
    (success, rvec, tvec, ascending inlier indices): dvs_solve_pnp_ransac's procedure.  -> dict"""
    out = stages123(P, xyz, ldesc, kps, kdesc)
    m = out["n_pairs"]
    out.update(status=OK, pnp_inliers=0, pnp_success=0, pnp_R=np.zeros((3, 3)), pnp_t=np.zeros(3), track=None, R=np.eye(3), t=np.zeros(3),
               pnp_inlier=np.zeros(m, np.uint8))
    if m < P.min_pairs:
        out["status"] = FEW_PAIRS
        return out
    ok, rvec, tvec, inl = pnp(out["obj"], out["img"], P.K4, P.pnp_iterations, P.pnp_reproj_err, P.pnp_confidence, P.seed)
    out.update(pnp_inliers=len(inl), pnp_success=int(bool(ok)), rvec=np.array(rvec, np.float64), tvec=np.array(tvec, np.float64))
    out["pnp_inlier"][np.asarray(inl, np.int64)] = 1
    if not ok or len(inl) < P.min_pnp_inliers or not (np.isfinite(rvec).all() and np.isfinite(tvec).all()):
        out["status"] = NO_POSE
        return out
    out["pnp_R"], out["pnp_t"] = rodrigues_pose(rvec, tvec)
    tr = mr.track(MP, out["pnp_R"], out["pnp_t"], xyz, ldesc, kps, kdesc)
    out["track"] = tr
    if tr["status"] == mr.OK and tr["n_inliers"] >= P.min_confirmed:
        out["R"], out["t"] = tr["R"], tr["t"]
    else:
        out["status"] = NOT_CONFIRMED
    return out


# ---------------------------------------------------------------------------------------------------- scenes
ROWS, COLS, FX, FY, CX, CY = 480, 640, 520.0, 515.0, 318.5, 241.25


def map_params(**kw):
    return mr.Params(ROWS, COLS, FX, FY, CX, CY, **kw)


def params(**kw):
    return Params([FX, FY, CX, CY], **kw)


def _flip(rng, desc, lo, hi):
    out = desc.copy()
    for k in range(len(out)):
        for b in rng.choice(256, int(rng.integers(lo, hi)), replace=False):
            out[k, b >> 3] ^= np.uint8(1 << (b & 7))
    return out


def scene(n_lm=3000, seed=21, n_distract=300, swap_frac=0.42, noise=0.4):
    """a room of n_lm landmarks seen from a pose 130 degrees and 2 m from the identity: a keypoint at every visible projection with
    sub-pixel noise and up to 8 flipped descriptor bits, n_distract keypoints with random descriptors anywhere, and a block of the visible
    landmarks whose keypoints' descriptors were rotated among themselves (their pairs are wrong) ->
    dict(P, MP, R_true, t_true, xyz, ldesc, ids, kps, kdesc, kp_truth (the landmark really under each keypoint, -1: a distractor), swapped)"""
    rng = np.random.default_rng(seed)
    MP = map_params()
    R_true = mr.rot("y", 130.0) @ mr.rot("x", -10.0); t_true = np.array([1.5, -0.3, 1.2])
    xyz = np.stack([rng.uniform(-6, 6, n_lm), rng.uniform(-2.5, 2.5, n_lm), rng.uniform(-6, 6, n_lm)], 1).astype(np.float32)
    c = (xyz.astype(np.float64) - t_true) @ R_true                       # R^T (X - t)
    with np.errstate(divide="ignore", invalid="ignore"):
        u = FX * c[:, 0] / c[:, 2] + CX; v = FY * c[:, 1] / c[:, 2] + CY
    vis = np.flatnonzero((c[:, 2] > 0.8) & (c[:, 2] < 12.0) & (u >= 4) & (u < COLS - 4) & (v >= 4) & (v < ROWS - 4))
    vis = rng.permutation(vis)                                           # keypoint order is not landmark order
    ldesc = mr.random_descriptors(rng, n_lm)
    kd = _flip(rng, ldesc[vis], 0, 9)
    n_swap = int(swap_frac * len(vis))
    kd[:n_swap] = np.roll(kd[:n_swap], 1, 0)                             # keypoint i carries the descriptor of the landmark under keypoint i - 1
    xy = np.stack([u[vis], v[vis]], 1) + rng.normal(0, noise, (len(vis), 2))
    dxy = np.stack([rng.uniform(0, COLS - 1, n_distract), rng.uniform(0, ROWS - 1, n_distract)], 1)
    kps = mr.keypoints(np.concatenate([xy, dxy]).astype(np.float32))
    kps["octave"] = rng.integers(0, 4, len(kps))
    kdesc = np.concatenate([kd, mr.random_descriptors(rng, n_distract)])
    truth = np.concatenate([vis, np.full(n_distract, -1)]).astype(np.int64)
    swapped = np.zeros(len(kps), bool); swapped[:n_swap] = True
    order = rng.permutation(len(kps))
    return dict(P=params(), MP=MP, R_true=R_true, t_true=t_true, xyz=xyz, ldesc=ldesc, ids=np.arange(n_lm, dtype=np.int64) * 2 + 7,
                kps=kps[order], kdesc=np.ascontiguousarray(kdesc[order]), kp_truth=truth[order], swapped=swapped[order])


def wrong_pairs(s, st):
    """which pairs of a stage-3 list name a landmark that is not the one under the keypoint"""
    return s["kp_truth"][st["kp_index"]] != st["lm_row"]


def random_frame(s, seed=5):
    """the scene's map with a frame of random descriptors"""
    rng = np.random.default_rng(seed)
    return dict(s, kdesc=mr.random_descriptors(rng, len(s["kps"])))


def cut_to_pairs(s, n_pairs):
    """the scene with only as many keypoints as give exactly n_pairs pairs: a prefix of the keypoints whose descriptor is their own landmark's"""
    good = np.flatnonzero((s["kp_truth"] >= 0) & ~s["swapped"])[:n_pairs]
    return dict(s, kps=s["kps"][good], kdesc=np.ascontiguousarray(s["kdesc"][good]), kp_truth=s["kp_truth"][good], swapped=s["swapped"][good])


def all_wrong(s):
    """every descriptor names another landmark than the one under its keypoint"""
    real = np.flatnonzero(s["kp_truth"] >= 0)
    kd = s["kdesc"].copy()
    own = np.flatnonzero((s["kp_truth"] >= 0) & ~s["swapped"])
    kd[own] = np.roll(kd[own], 1, 0)
    return dict(s, kps=s["kps"][real], kdesc=np.ascontiguousarray(kd[real]), kp_truth=s["kp_truth"][real], swapped=np.ones(len(real), bool))


# ---- stages 1-3 at the edges
def tie_scene(n_lm, n_kp, seed):
    """descriptors from a pool of six patterns with at most one of four chosen bits flipped: most distances are shared by many pairs, many
    rows are duplicates, so the lowest keypoint and the lowest landmark row decide -> (xyz, ldesc, kps, kdesc)"""
    rng = np.random.default_rng(seed)
    pool = mr.random_descriptors(rng, 6)
    bits = [3, 77, 130, 255]

    def draw(n):
        d = pool[rng.integers(0, 6, n)].copy()
        for i in range(n):
            b = int(rng.integers(0, 8))
            if b < 4:
                d[i, bits[b] >> 3] ^= np.uint8(1 << (bits[b] & 7))
        return d
    xyz = rng.uniform(-3, 3, (n_lm, 3)).astype(np.float32)
    kps = mr.keypoints(np.stack([rng.uniform(0, COLS - 1, n_kp), rng.uniform(0, ROWS - 1, n_kp)], 1).astype(np.float32))
    return xyz, draw(n_lm), kps, draw(n_kp)


def _with_bits(base, n, start=0):
    d = base.copy()
    for b in range(start, start + n):
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


def special_scene(P, seed=3):
    """one table with every crafted case (ratio_pct must be > 0, max_hamming >= 8) -> (xyz, ldesc, kps, kdesc, rows: name -> landmark rows)
    keypoints 0, 1:  A, B with B = A + 16 bits (others are >= 80 away from both)
      ratio_eq      hamming to A is a, to B is b with a * 100 == ratio_pct * b exactly: does not propose
      ratio_in      one bit more on B's side: proposes to A
    keypoint 2:  C.  at_max_m1 is max_hamming - 1 from C (proposes), at_max is max_hamming from C (does not)
    keypoint 3:  E.  crowd: 200 landmarks 1 + ((7 j + 3) mod 5) bits from E all propose to it; the lowest row of the smallest distance
                 (the crowd's second) is kept
    keypoint 4:  G.  dup: three landmarks with one descriptor 2 bits from G: the first row is kept.  not_finite: the same descriptor, at
                 d = 0 .. 1, with NaN / +inf / -inf coordinates, ahead of them in the table: never proposes, so dup wins"""
    rng = np.random.default_rng(seed)
    A, C_, E, G = mr.random_descriptors(rng, 4)
    B = _with_bits(A, 16, 100)
    # a = 3, b = 4 at ratio_pct 75: distances (a, b) to (A, B) need a + b >= 16 (triangle) — scale: a = 3 q, b = 4 q with q = 4: 12 + 16 = 28 >= 16
    g = math.gcd(P.ratio_pct, 100)
    a, b = 4 * (P.ratio_pct // g), 4 * (100 // g)                           # a * 100 == ratio_pct * b
    # a landmark x bits into the 16 that separate A and B and y bits elsewhere: d(A) = x + y, d(B) = 16 - x + y
    x = (a - b + 16) // 2; y = a - x
    assert 0 <= x <= 16 and y >= 0 and x + y == a and 16 - x + y == b and a < P.max_hamming
    eq = _with_bits(_with_bits(A, x, 100), y, 0)
    inn = _with_bits(_with_bits(A, x - 1, 100), y, 0)                       # one bit less towards B: d(A) = a - 1, d(B) = b + 1
    rows, ld, xyz = {}, [], []

    def add(name, descs, pos=None):
        rows[name] = list(range(len(ld), len(ld) + len(descs)))
        ld.extend(descs)
        xyz.extend(pos if pos is not None else [[0.5, 0.25, 2.0 + 0.01 * len(ld)]] * len(descs))
    add("ratio_eq", [eq]); add("ratio_in", [inn])
    add("at_max_m1", [_with_bits(C_, P.max_hamming - 1)]); add("at_max", [_with_bits(C_, P.max_hamming)])
    add("not_finite", [G, _with_bits(G, 1), G], [[np.nan, 0, 1], [0, np.inf, 1], [0, 0, -np.inf]])
    add("crowd", [_with_bits(E, 1 + (7 * j + 3) % 5, 3 * j % 200) for j in range(200)])
    add("dup", [_with_bits(G, 2, 40)] * 3)
    kd = np.stack([A, B, C_, E, G] + list(mr.random_descriptors(rng, 7)))
    kps = mr.keypoints(np.stack([np.arange(12) * 40.0 + 5, np.arange(12) * 30.0 + 7], 1).astype(np.float32))
    return np.array(xyz, np.float32), np.stack(ld), kps, kd, rows
