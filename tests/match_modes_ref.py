"""numpy statement of cv::BFMatcher(NORM_HAMMING) knnMatch / crossCheck / radiusMatch (restated from OpenCV 4.x's
batchDistance and radiusMatchImpl; parity unpinned) — the reference the matcher-mode tests compare against, bit for bit."""
import numpy as np

INT32_MAX = 2 ** 31 - 1


def distances(q, t, rows=256):
    """d[i, j] = Hamming distance of query row i to train row j (int64), brute force with np.unpackbits, in row blocks"""
    q = np.ascontiguousarray(q, np.uint8).reshape(-1, 32); t = np.ascontiguousarray(t, np.uint8).reshape(-1, 32)
    d = np.zeros((len(q), len(t)), np.int64)
    for b in range(0, len(q), rows):
        x = q[b:b + rows, None, :] ^ t[None, :, :]
        d[b:b + rows] = np.unpackbits(x, axis=2).sum(axis=2)
    return d


def knn(d, k):
    """(idx[nq, k], dist[nq, k]): first min(k, nt) train rows by (distance, train index); padding -1 / INT32_MAX"""
    nq, nt = d.shape
    idx = np.full((nq, k), -1, np.int32); dist = np.full((nq, k), INT32_MAX, np.int32)
    kk = min(k, nt)
    if kk and nq:
        key = d * (1 << 23) + np.arange(nt)[None, :]
        o = np.argsort(key, axis=1, kind="stable")[:, :kk]
        idx[:, :kk] = o
        dist[:, :kk] = np.take_along_axis(d, o, axis=1)
    return idx, dist


def cross(d):
    """(idx[nq], dist[nq]): query i keeps j = argmin_j d(i, .) if i = argmin_i d(., j) (np.argmin: first = lowest index on ties)"""
    nq, nt = d.shape
    idx = np.full(nq, -1, np.int32); dist = np.full(nq, INT32_MAX, np.int32)
    if nq == 0 or nt == 0:
        return idx, dist
    fwd = d.argmin(axis=1); bwd = d.argmin(axis=0)
    keep = bwd[fwd] == np.arange(nq)
    idx[keep] = fwd[keep]; dist[keep] = d[np.arange(nq), fwd][keep]
    return idx, dist


def radius(d, max_distance, order):
    """(offsets int64[nq + 1], idx, dist): per query the pairs with (float)d <= max_distance in train order, then permuted by
    order(dists) -> the permutation std::sort(DMatch::operator<) applies (distance only; the tests pass the oracle's real std::sort)"""
    nq = d.shape[0]
    offs = np.zeros(nq + 1, np.int64); I = []; D = []
    for i in range(nq):
        js = np.nonzero(d[i].astype(np.float32) <= np.float32(max_distance))[0]
        ds = d[i, js]
        p = np.asarray(order(ds.astype(np.int32)), np.int64) if len(js) else np.zeros(0, np.int64)
        I.append(js[p]); D.append(ds[p])
        offs[i + 1] = offs[i] + len(js)
    cat = (lambda a: np.concatenate(a).astype(np.int32)) if nq else (lambda a: np.zeros(0, np.int32))
    return offs, cat(I), cat(D)


def std_sort_order(oracle):
    """the permutation the real std::sort leaves for a distance-only comparison: the oracle's orc_std_sort_nodes with equal ulx"""
    def order(ds):
        ds = np.ascontiguousarray(ds, np.int32); n = len(ds)
        ulx = np.zeros(n, np.int32); perm = np.zeros(n, np.int32)
        oracle.lib().orc_std_sort_nodes(ds.ctypes.data, ulx.ctypes.data, n, perm.ctypes.data)
        return perm
    return order


def tie_heavy(kind, n, seed):
    """descriptor sets whose distances tie a lot"""
    rng = np.random.default_rng(seed)
    if kind == "three":       # only 3 distinct rows: long runs of equal distances
        base = rng.integers(0, 256, (3, 32), dtype=np.uint8)
        return base[rng.integers(0, 3, n)]
    if kind == "zeros_ones":  # all-zero and all-ones rows (+ a few random)
        x = np.where(rng.random((n, 1)) < 0.5, 0, 255).astype(np.uint8).repeat(32, axis=1)
        x[::7] = rng.integers(0, 256, (len(x[::7]), 32), dtype=np.uint8)
        return x
    if kind == "near":        # near-duplicates of a few rows: small distances, many equal
        base = rng.integers(0, 256, (5, 32), dtype=np.uint8)
        x = base[rng.integers(0, 5, n)].copy()
        flip = rng.integers(0, 256, n)
        x[np.arange(n), flip // 8] ^= (1 << (flip % 8)).astype(np.uint8)
        return x
    raise ValueError(kind)
