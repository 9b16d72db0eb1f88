"""Backend::syncCallback (backend.cpp:709-832), the BA window (:892-945), updateOptimizedResults (:1356-1392) and pruneLandmarks
(:1249-1322) restated over plain dicts and lists, in the reference's statement order.  landmark_database_ is one dict per class id,
iterated in ASCENDING id (the handle's stated order; the reference's unordered_map order is not reproduced).  Triangulation is
triangulate_ref's; the reprojection error is oracle_bindings.associate's arithmetic (orc_associate) written out in Python floats."""
import math
import numpy as np
import triangulate_ref as tr

f32 = np.float32
_POPCOUNT = np.array([bin(v).count("1") for v in range(256)], np.int64)


def quat_to_R(q_xyzw):
    """extractPoseFromTransform (:1194-1215)"""
    qx, qy, qz, qw = (float(v) for v in q_xyzw)
    norm = math.sqrt(qw * qw + qx * qx + qy * qy + qz * qz)
    qw /= norm; qx /= norm; qy /= norm; qz /= norm
    return np.array([1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qw * qz), 2 * (qx * qz + qw * qy),
                     2 * (qx * qy + qw * qz), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qw * qx),
                     2 * (qx * qz - qw * qy), 2 * (qy * qz + qw * qx), 1 - 2 * (qx * qx + qy * qy)], np.float64)


def categorize(pixel, detections):
    """categorizeObservation (:1011-1029): pixel = (float32, float32); detections = [(cx, cy, w, h, class_id)]; 0 = unlabeled"""
    x, y = float(f32(pixel[0])), float(f32(pixel[1]))
    for cx, cy, w, h, cls in detections:
        if x >= cx - w / 2 and x <= cx + w / 2 and y >= cy - h / 2 and y <= cy + h / 2:
            return cls
    return 0


def reprojection_error(px, X, R, t, fx, fy, cx, cy):
    """|pixel - reprojectPoint(X)| (:1100-1103, :1153-1173): double camera coordinates, float pixel, float difference, double norm"""
    d0, d1, d2 = float(X[0]) - t[0], float(X[1]) - t[1], float(X[2]) - t[2]
    c0 = R[0] * d0 + R[3] * d1 + R[6] * d2
    c1 = R[1] * d0 + R[4] * d1 + R[7] * d2
    c2 = R[2] * d0 + R[5] * d1 + R[8] * d2
    u, v = f32(-1.0), f32(-1.0)
    if not c2 <= 0:
        u, v = f32(fx * c0 / c2 + cx), f32(fy * c1 / c2 + cy)
    dx, dy = float(f32(px[0]) - u), float(f32(px[1]) - v)
    return math.sqrt(dx * dx + dy * dy)


def hamming(a, b):
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


def prune_rule(count, last_seen_ns, now_ns, min_obs=2, max_age=20.0):
    """:1260-1264 with the age read as (double)(now - last_seen) / 1e9 (unpinned against rclcpp::Duration::seconds())"""
    return count < min_obs and float(now_ns - last_seen_ns) / 1e9 > max_age


class BackendRef:
    def __init__(self, fx, fy, cx, cy, filtered=(), max_desc=50.0, max_reproj=5.0, window=5, min_obs=2, max_age=20.0):
        self.K = (float(fx), float(fy), float(cx), float(cy))
        self.filtered = set(filtered); self.max_desc, self.max_reproj = max_desc, max_reproj
        self.window_size, self.min_obs, self.max_age = window, min_obs, max_age
        self.db = {}                 # landmark_database_: class -> {id: dict(id, cls, pos float32[3], desc, obs_ids, count, last_seen)}
        self.obs = []                # all_observations_: dict(id, frame, px float32[2], desc, cls, lm)
        self.kfs = []                # keyframes_: dict(frame, R[9], t[3], stamp, obs_ids)
        self.next_obs = 0; self.next_lm = 0
        self.ties = 0                # candidates that tied exactly with the winner (the stated deviation would show here)
        self.last_best = {}          # class -> per-observation landmark id or -1, of the last keyframe
        self._rows = {}

    # ---- :1064-1120
    def associate(self, px, desc, cls, R, t):
        ids, descs = self._class_rows(cls)
        dist = _POPCOUNT[np.bitwise_xor(descs, desc[None, :])].sum(1) if len(ids) else np.zeros(0, np.int64)
        cands = [ids[j] for j in np.nonzero(dist.astype(np.float32) < self.max_desc)[0]]          # ascending id (:1068-1077)
        best, best_e = -1, float("inf")
        for lid in cands:
            e = reprojection_error(px, self.db[cls][lid]["pos"], R, t, *self.K)
            if e < self.max_reproj and e == best_e:
                self.ties += 1
            if e < self.max_reproj and e < best_e:
                best, best_e = lid, e
        return best

    def _class_rows(self, cls):
        """ids (ascending) and descriptor rows of one class; descriptors never change, so the rows are rebuilt only when the class's size does"""
        d = self.db.get(cls, {})
        c = self._rows.get(cls)
        if c is None or c[2] != (len(d), max(d) if d else -1):
            ids = sorted(d)
            c = (ids, np.array([d[i]["desc"] for i in ids], np.uint8).reshape(-1, 32), (len(d), max(d) if d else -1))
            self._rows[cls] = c
        return c[0], c[1]

    # ---- :439-613 through triangulate_ref, from all_observations_ / keyframes_ as they stand
    def triangulate(self, lm):
        if len(lm["obs_ids"]) < 2:
            return False
        by_id = {o["id"]: o for o in self.obs}
        kf_of = {}
        for k, kf in enumerate(self.kfs):
            kf_of.setdefault(kf["frame"], k)
        vkf, vpx = [], []
        for oid in lm["obs_ids"]:
            o = by_id.get(oid)
            if o is None:
                continue
            vkf.append(kf_of.get(o["frame"], -1)); vpx.append(o["px"])
        if not vkf:
            return False
        R = np.array([kf["R"] for kf in self.kfs]); t = np.array([kf["t"] for kf in self.kfs])
        out, st = tr.triangulate(R, t, *self.K, [0, len(vkf)], np.array(vkf, np.int32), np.array(vpx, f32).reshape(-1, 2), lm["pos"].reshape(1, 3))
        if st[0] == tr.UPDATED:
            lm["pos"] = out[0].copy()
            return True
        return False

    # ---- :709-832
    def add_keyframe(self, frame_id, stamp, translation, rotation_xyzw, landmark_xyz, obs_pixels, obs_desc, detections=()):
        stamp_ns = int(stamp[0]) * 10**9 + int(stamp[1])
        R = quat_to_R(rotation_xyzw); t = np.array(translation, np.float64)
        kf = dict(frame=int(frame_id), R=R, t=t, stamp=stamp_ns, obs_ids=[])
        new_obs, new_lms = [], {}
        res = dict(n_kept=0, n_filtered=0, n_associated=0, n_created=0, n_moved=0, first_observation_id=self.next_obs, first_landmark_id=self.next_lm)
        moved = set(); self.last_best = {}
        for i in range(len(obs_pixels)):
            px = np.array(obs_pixels[i], np.float64).astype(f32); desc = np.array(obs_desc[i], np.uint8)
            cls = categorize(px, detections)
            if cls in self.filtered:
                res["n_filtered"] += 1
                continue
            o = dict(id=self.next_obs, frame=int(frame_id), px=px, desc=desc, cls=cls, lm=-1)
            kf["obs_ids"].append(self.next_obs); self.next_obs += 1
            lid = self.associate(px, desc, cls, R, t)
            self.last_best.setdefault(cls, []).append(lid)
            if lid != -1:
                o["lm"] = lid
                lm = self.db[cls][lid]
                lm["count"] += 1; lm["last_seen"] = stamp_ns; lm["obs_ids"].append(o["id"])
                if self.triangulate(lm):
                    moved.add(lid)
                res["n_associated"] += 1
            else:
                lid = self.next_lm; self.next_lm += 1
                new_lms.setdefault(cls, {})[lid] = dict(id=lid, cls=cls, pos=np.array(landmark_xyz[i], np.float64).astype(f32), desc=desc, obs_ids=[o["id"]],
                                                        count=1, last_seen=stamp_ns)
                o["lm"] = lid
                res["n_created"] += 1
            new_obs.append(o)
        self.kfs.append(kf)
        self.obs.extend(new_obs)
        for cls, lms in new_lms.items():
            self.db.setdefault(cls, {}).update(lms)
        res["n_kept"] = len(new_obs); res["n_moved"] = len(moved)
        return res

    # ---- :892-945
    def window(self):
        w = min(self.window_size, len(self.kfs))
        kfs = self.kfs[len(self.kfs) - w:]
        ids = set()
        for kf in kfs:
            ids.update(kf["obs_ids"])
        obs, lm_keys = [], set()
        for o in self.obs:
            if o["id"] in ids:
                lm_keys.add((o["lm"], o["cls"]))
                obs.append(o)
        lms = [self.db[cls][lid] for lid, cls in sorted(lm_keys)]
        return kfs, obs, lms

    # ---- :1356-1392
    def apply_optimized(self, poses, landmarks):
        for fid, (R, t) in poses.items():
            for kf in self.kfs:
                if kf["frame"] == int(fid):
                    kf["R"] = np.array(R, np.float64).reshape(9).copy(); kf["t"] = np.array(t, np.float64).reshape(3).copy()
                    break
        for (lid, cls), pos in landmarks.items():
            if cls in self.db and lid in self.db[cls]:
                self.db[cls][lid]["pos"] = np.array(pos, np.float64).astype(f32)

    # ---- :1249-1322
    def prune(self, now):
        now_ns = int(now[0]) * 10**9 + int(now[1])
        to_remove = [(lid, cls) for cls in sorted(self.db) for lid in sorted(self.db[cls])
                     if prune_rule(self.db[cls][lid]["count"], self.db[cls][lid]["last_seen"], now_ns, self.min_obs, self.max_age)]
        removed_obs = 0
        self._rows = {}
        for lid, cls in to_remove:
            gone = set(self.db[cls][lid]["obs_ids"])
            del self.db[cls][lid]
            keep = []
            for o in self.obs:
                if o["id"] in gone or o["lm"] == lid:
                    removed_obs += 1
                else:
                    keep.append(o)
            self.obs = keep
            for kf in self.kfs:
                kf["obs_ids"] = [i for i in kf["obs_ids"] if i not in gone]
        return len(to_remove), removed_obs

    # ---- the tables as the handle's getters return them
    def landmark_table(self):
        lms = sorted((lm for d in self.db.values() for lm in d.values()), key=lambda lm: lm["id"])
        offs = np.zeros(len(lms) + 1, np.int64)
        for k, lm in enumerate(lms):
            offs[k + 1] = offs[k] + len(lm["obs_ids"])
        return dict(id=np.array([lm["id"] for lm in lms], np.uint64), class_id=np.array([lm["cls"] for lm in lms], np.int32),
                    xyz=np.array([lm["pos"] for lm in lms], f32).reshape(-1, 3), desc=np.array([lm["desc"] for lm in lms], np.uint8).reshape(-1, 32),
                    observation_count=np.array([lm["count"] for lm in lms], np.int32), last_seen_ns=np.array([lm["last_seen"] for lm in lms], np.int64),
                    obs_offsets=offs, obs_ids=np.array([i for lm in lms for i in lm["obs_ids"]], np.uint64))

    def observation_table(self):
        o = self.obs
        return dict(id=np.array([x["id"] for x in o], np.uint64), frame_id=np.array([x["frame"] for x in o], np.uint64),
                    px=np.array([x["px"] for x in o], f32).reshape(-1, 2), desc=np.array([x["desc"] for x in o], np.uint8).reshape(-1, 32),
                    class_id=np.array([x["cls"] for x in o], np.int32), landmark_id=np.array([x["lm"] for x in o], np.uint64))

    def keyframe_table(self):
        k = self.kfs
        offs = np.zeros(len(k) + 1, np.int64)
        for j, kf in enumerate(k):
            offs[j + 1] = offs[j] + len(kf["obs_ids"])
        return dict(frame_id=np.array([x["frame"] for x in k], np.uint64), stamp_ns=np.array([x["stamp"] for x in k], np.int64),
                    R=np.array([x["R"] for x in k], np.float64).reshape(-1, 3, 3), t=np.array([x["t"] for x in k], np.float64).reshape(-1, 3),
                    obs_offsets=offs, obs_ids=np.array([i for x in k for i in x["obs_ids"]], np.uint64))

    def window_table(self):
        kfs, obs, lms = self.window()
        index = {lm["id"]: k for k, lm in enumerate(lms)}
        return dict(kf_frame_id=np.array([x["frame"] for x in kfs], np.uint64), kf_R=np.array([x["R"] for x in kfs], np.float64).reshape(-1, 3, 3),
                    kf_t=np.array([x["t"] for x in kfs], np.float64).reshape(-1, 3), obs_px=np.array([x["px"] for x in obs], f32).reshape(-1, 2),
                    obs_landmark_id=np.array([x["lm"] for x in obs], np.uint64), obs_class=np.array([x["cls"] for x in obs], np.int32),
                    obs_frame_id=np.array([x["frame"] for x in obs], np.uint64), obs_lm_index=np.array([index[x["lm"]] for x in obs], np.int32),
                    lm_id=np.array([x["id"] for x in lms], np.uint64), lm_class=np.array([x["cls"] for x in lms], np.int32),
                    lm_xyz=np.array([x["pos"] for x in lms], f32).reshape(-1, 3))


# ---- the synthetic scene of the GPU tests -----------------------------------------------------------------------------------------
FX = FY = 500.0; CX, CY = 320.0, 240.0
Q_Z180 = (0.0, 0.0, 1.0, 0.0)   # R = diag(-1, -1, 1): with t in the x-y plane, x_cam = R X + t (triangulate) and R^T (X - t) (reprojectPoint) agree
PERSON, CHAIR, TABLE = 1, 2, 3


def make_scene(seed=7, npoints=200, nkf=10, pixel_noise=0.3, position_noise=0.03, step=(0.22, 0.04)):
    """-> list of keyframes dict(frame_id, stamp, t, q, xyz, px, desc, det): world points with random 256-bit descriptors (0-3 bits flipped
    per view), a camera stepping sideways, three detections per keyframe: PERSON (filtered by the tests), CHAIR and TABLE overlapping"""
    rng = np.random.default_rng(seed)
    X = np.stack([rng.uniform(-1.6, 2.8, npoints), rng.uniform(-1.2, 1.4, npoints), rng.uniform(2.2, 4.5, npoints)], 1)
    D = rng.integers(0, 256, (npoints, 32), dtype=np.uint8)
    out = []
    for k in range(nkf):
        t = np.array([step[0] * k, step[1] * k, 0.0])
        xc = np.stack([-X[:, 0] + t[0], -X[:, 1] + t[1], X[:, 2]], 1)
        u = FX * xc[:, 0] / xc[:, 2] + CX; v = FY * xc[:, 1] / xc[:, 2] + CY
        vis = np.nonzero((u > 8) & (u < 632) & (v > 8) & (v < 472))[0]
        vis = vis[rng.permutation(len(vis))]
        px = np.stack([u[vis], v[vis]], 1) + rng.normal(0, pixel_noise, (len(vis), 2))
        desc = D[vis].copy()
        for r in range(len(vis)):
            for b in rng.choice(256, rng.integers(0, 4), replace=False):
                desc[r, b >> 3] ^= np.uint8(1 << (b & 7))
        xyz = X[vis] + rng.normal(0, position_noise, (len(vis), 3))
        det = [(120.0 + 6 * k, 240.0, 90.0, 200.0, PERSON), (400.0 - 9 * k, 200.0, 220.0, 180.0, CHAIR), (450.0 - 9 * k, 260.0, 200.0, 200.0, TABLE)]
        out.append(dict(frame_id=100 + k, stamp=(10 + 3 * k, 500000000), t=t, q=Q_Z180, xyz=xyz, px=px, desc=desc, det=det))
    return out
