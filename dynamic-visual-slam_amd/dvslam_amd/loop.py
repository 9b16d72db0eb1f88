"""Loop candidates: a keyframe database with a direct index and node-guided matching over dvs_loop_* (include/dvslam_hip.h, "loop
candidates"; csrc/loop.hip).  No CPU fallback: the vocabulary it is built over needs the device."""
import ctypes as C
import numpy as np
from ._lib import check, ptr, LoopMatchParams
from .bow import _rows

INT32_MAX = 2 ** 31 - 1
# mirrors of csrc/loop.hip's constants (tests/test_loop_cpu.py compares them with the source text): the tests size their segments and
# query blocks by them
MATCH_TILE_ROWS = 128
MATCH_QUERY_BLOCK = 64


def _params(max_distance, ratio):
    return LoopMatchParams(int(max_distance), int(ratio[0]), int(ratio[1]))


class LoopDatabase:
    """LoopDatabase(vocabulary, di_levels): add(features) -> entry id, query(...) -> [(Id, Score)] as OrbDatabase; retrieve_features(id)
    -> [(node id, [feature indices])]; match(features, entry_ids) -> (train_idx [c][n], dist [c][n], n_matches [c]); detect(features,
    max_results, max_id) -> (ids, scores, n_matches, train_idx, dist) in one call.  Unmatched rows: train_idx -1, dist INT32_MAX."""

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
