"""Loop candidates: a keyframe database with a direct index and node-guided matching over dvs_loop_* (include/dvslam_hip.h, "loop
candidates"; csrc/loop.hip), and the rigid 3D-3D verification of the candidates ("loop verification"; csrc/loop_verify.hip).  No CPU fallback: the vocabulary it is built over needs the device."""
import ctypes as C
import numpy as np
from ._lib import check, ptr, LoopMatchParams, LoopVerifyParams, LOOP_VERIFY_RESULT
from .bow import _rows

INT32_MAX = 2 ** 31 - 1
# mirrors of csrc/loop.hip's constants (tests/test_loop_cpu.py compares them with the source text): the tests size their segments and
# query blocks by them
MATCH_TILE_ROWS = 128
MATCH_QUERY_BLOCK = 64


def _points(points):
    return np.ascontiguousarray(points, np.float32).reshape(-1, 3)


def _params(max_distance, ratio):
    return LoopMatchParams(int(max_distance), int(ratio[0]), int(ratio[1]))


class LoopDatabase:
    """LoopDatabase(vocabulary, di_levels): add(features) -> entry id, query(...) -> [(Id, Score)] as OrbDatabase; retrieve_features(id)
    -> [(node id, [feature indices])]; match(features, entry_ids) -> (train_idx [c][n], dist [c][n], n_matches [c]); detect(features,
    max_results, max_id) -> (ids, scores, n_matches, train_idx, dist) in one call.  Unmatched rows: train_idx -1, dist INT32_MAX.
    set_points(id, xyz) / get_points(id); verify(points, entry_ids, train_idx, LoopVerifyParams) -> (records, inlier masks);
    detect_verify(features, points, LoopVerifyParams, ...) -> detect's outputs plus the records and masks, in one call."""

    def __init__(self, vocabulary, di_levels=0):
        self._voc = vocabulary            # the handle borrows the vocabulary: keep it alive
        self._L = vocabulary._L
        self._h = None
        h = C.c_void_p()
        check(self._L.dvs_loop_db_create(vocabulary._h, di_levels, C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._L.dvs_loop_db_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def size(self):
        return self._L.dvs_loop_db_size(self._h)

    def di_levels(self):
        return self._L.dvs_loop_db_di_levels(self._h)

    def clear(self):
        check(self._L.dvs_loop_db_clear(self._h))

    def add(self, features):
        f = _rows(features)
        e = C.c_int32(-1)
        check(self._L.dvs_loop_db_add(self._h, ptr(f), len(f), C.byref(e)))
        return e.value

    def add_device(self, d_desc, d_n, stride_rows, nframes):
        e = C.c_int32(-1)
        check(self._L.dvs_loop_db_add_device(self._h, d_desc, d_n, stride_rows, nframes, C.byref(e)))
        return e.value

    def _cap(self, max_results):
        size = self.size()
        return size if max_results <= 0 else min(max_results, size)

    def query_arrays(self, features, max_results=0, max_id=-1):
        """(ids int32[], scores float64[])"""
        f = _rows(features)
        cap = self._cap(max_results)
        ids = np.zeros(max(cap, 1), np.int32); scores = np.zeros(max(cap, 1), np.float64)
        n = C.c_int32()
        check(self._L.dvs_loop_db_query(self._h, ptr(f), len(f), max_results, max_id, ptr(ids), ptr(scores), cap, C.byref(n)))
        return ids[:n.value].copy(), scores[:n.value].copy()

    def query(self, features, max_results=0, max_id=-1):
        ids, scores = self.query_arrays(features, max_results, max_id)
        return [(int(i), float(s)) for i, s in zip(ids, scores)]

    def query_device(self, d_desc, d_n, stride_rows, max_results, max_id, d_ids, d_scores, cap, d_n_results):
        check(self._L.dvs_loop_db_query_device(self._h, d_desc, d_n, stride_rows, max_results, max_id, d_ids, d_scores, cap, d_n_results))

    def retrieve_features(self, entry_id):
        """DBoW2's retrieveFeatures: [(node id, [feature indices])] in ascending node id"""
        nn, m = C.c_int32(), C.c_int32()
        code = self._L.dvs_loop_db_get_features(self._h, entry_id, None, None, None, 0, 0, C.byref(nn), C.byref(m))
        if code not in (0, -3):
            check(code)
        nodes = np.zeros(max(nn.value, 1), np.int32); offs = np.zeros(nn.value + 1, np.int32); feats = np.zeros(max(m.value, 1), np.int32)
        check(self._L.dvs_loop_db_get_features(self._h, entry_id, ptr(nodes), ptr(offs), ptr(feats), nn.value, m.value, C.byref(nn), C.byref(m)))
        return [(int(nodes[s]), feats[offs[s]:offs[s + 1]].tolist()) for s in range(nn.value)]

    def get_descriptors(self, entry_id):
        n = C.c_int32()
        code = self._L.dvs_loop_db_get_descriptors(self._h, entry_id, None, 0, C.byref(n))
        if code not in (0, -3):
            check(code)
        rows = np.zeros((max(n.value, 1), 32), np.uint8)
        check(self._L.dvs_loop_db_get_descriptors(self._h, entry_id, ptr(rows), n.value, C.byref(n)))
        return rows[:n.value].copy()

    def match(self, features, entry_ids, max_distance=50, ratio=(3, 4)):
        """(train_idx int32[c, n], dist int32[c, n], n_matches int32[c]) of the guided match against every listed entry"""
        f = _rows(features)
        ids = np.ascontiguousarray(entry_ids, np.int32).reshape(-1)
        c, n = len(ids), len(f)
        train = np.full((c, n), -1, np.int32); dist = np.full((c, n), INT32_MAX, np.int32); nm = np.zeros(c, np.int32)
        p = _params(max_distance, ratio)
        check(self._L.dvs_loop_db_match(self._h, ptr(f), n, ptr(ids) if c else None, c, C.byref(p), ptr(train), ptr(dist), ptr(nm)))
        return train, dist, nm

    def match_device(self, d_desc, d_n, stride_rows, d_entry_ids, d_n_cand, cap_cand, d_train_idx, d_dist, d_n_matches, max_distance=50, ratio=(3, 4)):
        p = _params(max_distance, ratio)
        check(self._L.dvs_loop_db_match_device(self._h, d_desc, d_n, stride_rows, d_entry_ids, d_n_cand, cap_cand, C.byref(p), d_train_idx, d_dist,
                                               d_n_matches))

    def detect(self, features, max_results=4, max_id=-1, max_distance=50, ratio=(3, 4)):
        """one transform, the query and the guided match of its results in one enqueue and one read-back:
        (ids int32[r], scores float64[r], n_matches int32[r], train_idx int32[r, n], dist int32[r, n])"""
        f = _rows(features)
        n, cap = len(f), self._cap(max_results)
        ids = np.zeros(max(cap, 1), np.int32); scores = np.zeros(max(cap, 1), np.float64); nm = np.zeros(max(cap, 1), np.int32)
        train = np.full((max(cap, 1), n), -1, np.int32); dist = np.full((max(cap, 1), n), INT32_MAX, np.int32)
        r = C.c_int32()
        p = _params(max_distance, ratio)
        check(self._L.dvs_loop_db_detect(self._h, ptr(f), n, max_results, max_id, C.byref(p), ptr(ids), ptr(scores), ptr(nm), ptr(train), ptr(dist), cap,
                                         C.byref(r)))
        r = r.value
        return ids[:r].copy(), scores[:r].copy(), nm[:r].copy(), train[:r].copy(), dist[:r].copy()

    def detect_device(self, d_desc, d_n, stride_rows, max_results, max_id, d_ids, d_scores, d_n_matches, d_train_idx, d_dist, cap, d_n_results,
                      max_distance=50, ratio=(3, 4)):
        p = _params(max_distance, ratio)
        check(self._L.dvs_loop_db_detect_device(self._h, d_desc, d_n, stride_rows, max_results, max_id, C.byref(p), d_ids, d_scores, d_n_matches,
                                                d_train_idx, d_dist, cap, d_n_results))

    # ---- loop verification: 3D points per entry, rigid 3D-3D RANSAC over the candidates (include/dvslam_hip.h, "loop verification") ----
    def set_points(self, entry_id, points):
        """the entry's 3D points, float32 [rows of the entry][3] in its camera frame; a row without depth is any invalid point (NaN)"""
        p = _points(points)
        check(self._L.dvs_loopv_db_set_points(self._h, entry_id, ptr(p), len(p)))

    def set_points_device(self, first_entry_id, d_xyz, d_n, stride_rows, nframes):
        check(self._L.dvs_loopv_db_set_points_device(self._h, first_entry_id, d_xyz, d_n, stride_rows, nframes))

    def get_points(self, entry_id):
        n = C.c_int32()
        code = self._L.dvs_loopv_db_get_points(self._h, entry_id, None, 0, C.byref(n))
        if code not in (0, -3):
            check(code)
        pts = np.zeros((max(n.value, 1), 3), np.float32)
        check(self._L.dvs_loopv_db_get_points(self._h, entry_id, ptr(pts), n.value, C.byref(n)))
        return pts[:n.value].copy()

    def verify(self, points, entry_ids, train_idx, params):
        """(results LOOP_VERIFY_RESULT[c], inlier_mask uint8[c, n]) for the query's points float32 [n][3] and train_idx int32 [c][n] of a match"""
        p = _points(points)
        ids = np.ascontiguousarray(entry_ids, np.int32).reshape(-1)
        c, n = len(ids), len(p)
        train = np.ascontiguousarray(train_idx, np.int32).reshape(c, n)
        res = np.zeros(max(c, 1), LOOP_VERIFY_RESULT); mask = np.zeros((max(c, 1), n), np.uint8)
        check(self._L.dvs_loopv_db_verify(self._h, ptr(p), n, ptr(ids) if c else None, c, ptr(train), C.byref(params), ptr(res), ptr(mask)))
        return res[:c].copy(), mask[:c].copy()

    def verify_device(self, d_xyz_query, d_n, stride_rows, d_entry_ids, d_n_cand, cap_cand, d_train_idx, params, d_results, d_inlier_mask):
        check(self._L.dvs_loopv_db_verify_device(self._h, d_xyz_query, d_n, stride_rows, d_entry_ids, d_n_cand, cap_cand, d_train_idx, C.byref(params),
                                                d_results, d_inlier_mask))

    def detect_verify(self, features, points, params, max_results=4, max_id=-1, max_distance=50, ratio=(3, 4)):
        """detect and the verification of its results in one enqueue and one read-back:
        (ids, scores, n_matches, train_idx, dist, results LOOP_VERIFY_RESULT[r], inlier_mask uint8[r, n])"""
        f = _rows(features); x = _points(points)
        assert len(x) == len(f), "one 3D point per descriptor row"
        n, cap = len(f), self._cap(max_results)
        k = max(cap, 1)
        ids = np.zeros(k, np.int32); scores = np.zeros(k, np.float64); nm = np.zeros(k, np.int32)
        train = np.full((k, n), -1, np.int32); dist = np.full((k, n), INT32_MAX, np.int32)
        res = np.zeros(k, LOOP_VERIFY_RESULT); mask = np.zeros((k, n), np.uint8)
        r = C.c_int32()
        p = _params(max_distance, ratio)
        check(self._L.dvs_loopv_db_detect_verify(self._h, ptr(f), ptr(x), n, max_results, max_id, C.byref(p), C.byref(params), ptr(ids), ptr(scores),
                                                ptr(nm), ptr(train), ptr(dist), ptr(res), ptr(mask), cap, C.byref(r)))
        r = r.value
        return ids[:r].copy(), scores[:r].copy(), nm[:r].copy(), train[:r].copy(), dist[:r].copy(), res[:r].copy(), mask[:r].copy()
