"""Reference of the masked ORB extraction (INTEGRATION.md §B1 "Keep masks"), composed from the CPU oracle's own stage functions:
the unmasked OracleORB.extract gives the pyramid, the blurred levels and the per-level FAST candidates (vToDistributeKeys,
ORBextractor.cpp:781-877); the candidates are filtered by the keep rule; the rest follows oracle/orb_oracle.cpp:267-309 stage by
stage — orc_distribute (DistributeOctTree), + minBorder, orc_ic_angle on the level, orc_descriptor on the blurred level, size /
octave, and the level-0 scaling.  A level with masked keypoints always had unmasked ones (its candidates are a subset), so its
blurred image exists in the unmasked run."""
import ctypes as C
import numpy as np
from oracle_bindings import KP_DTYPE, _p

EDGE_THRESHOLD, MIN_BORDER, PATCH_SIZE = 19, 16, 31


def keep(cand, scale_l, mask):
    """keep flags of region-relative candidates (int32 [n, 3]) on a level of scale `scale_l`: the pixel under the coordinates the
    keypoint would carry, X = float32(cx + minBorderX) * float32(scale) (one float32 multiply), floored and clamped to the mask"""
    rows, cols = mask.shape
    s = np.float32(scale_l)
    X = (cand[:, 0] + MIN_BORDER).astype(np.float32) * s
    Y = (cand[:, 1] + MIN_BORDER).astype(np.float32) * s
    assert X.dtype == np.float32 and Y.dtype == np.float32
    xi = np.minimum(cols - 1, np.floor(X).astype(np.int64))
    yi = np.minimum(rows - 1, np.floor(Y).astype(np.int64))
    return mask[yi, xi] != 0


def distribute(o, kept, w, h, N):
    """orc_distribute: the oracle's DistributeOctTree on region-relative candidates, in candidate order"""
    xys = np.ascontiguousarray(kept if len(kept) else np.zeros((1, 3), np.int32), np.int32)
    out = np.zeros((N + 64, 3), np.int32)
    n = o.L.orc_distribute(_p(xys), len(kept), MIN_BORDER, w - EDGE_THRESHOLD + 3, MIN_BORDER, h - EDGE_THRESHOLD + 3, N, _p(out), len(out))
    assert n >= 0
    return out[:n]


class MaskedRef:
    """the unmasked oracle run of one image, kept for any number of masks"""

    def __init__(self, oracle, img, nfeatures, scale_factor=1.2, nlevels=8, ini_th=20, min_th=7):
        self.o = oracle.OracleORB(nfeatures, scale_factor, nlevels, ini_th, min_th)
        self.img = np.ascontiguousarray(img)
        self.result = self.o.extract(self.img)
        assert self.result[0] >= 0
        self.nlevels = nlevels
        self.scale, _, self.fpl, _ = self.o.tables()
        self.cand = [self.o.candidates(l) for l in range(nlevels)]
        self._lev = {}

    def level(self, l, blurred):
        if (l, blurred) not in self._lev:
            self._lev[(l, blurred)] = self.o.level(l, blurred)
        return self._lev[(l, blurred)]

    def filtered_candidates(self, mask):
        return [c[keep(c, self.scale[l], mask)] for l, c in enumerate(self.cand)]

    def extract(self, mask):
        """(n, keypoints, descriptors) of the masked call, in the reference's output order (level-major)"""
        rows, cols = self.img.shape
        assert mask.shape == (rows, cols) and mask.dtype == np.uint8
        kps, descs = [], []
        for l, kept in enumerate(self.filtered_candidates(mask)):
            w, h = self.o.level_size(cols, rows, l)
            lk = distribute(self.o, kept, w, h, int(self.fpl[l]))
            if not len(lk):
                continue
            lev, blur = self.level(l, False), self.level(l, True)
            assert lev is not None and blur is not None, f"level {l}: masked keypoints on a level the unmasked run left empty"
            s = np.float32(self.scale[l])
            k = np.zeros(len(lk), KP_DTYPE)
            d = np.zeros((len(lk), 32), np.uint8)
            for i, (x, y, r) in enumerate(lk):
                fx, fy = float(x + MIN_BORDER), float(y + MIN_BORDER)
                a = self.o.L.orc_ic_angle(_p(lev), w, fx, fy)
                self.o.L.orc_descriptor(_p(blur), w, fx, fy, C.c_float(a), _p(d[i]))
                k[i] = (fx, fy, float(int(np.float32(PATCH_SIZE) * s)), a, float(r), l, -1)
            if l != 0:
                k["x"] = k["x"] * s
                k["y"] = k["y"] * s
            kps.append(k); descs.append(d)
        if not kps:
            return 0, np.zeros(0, KP_DTYPE), np.zeros((0, 32), np.uint8)
        k = np.concatenate(kps); d = np.concatenate(descs)
        return len(k), k, d
