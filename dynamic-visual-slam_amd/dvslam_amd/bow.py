"""Place recognition: thin mirrors of DBoW2's OrbVocabulary / OrbDatabase over dvs_bow_* (include/dvslam_hip.h, csrc/bow.hip), as the
reference's test/test_dbow2_integration.cpp uses them, and OrbVocabulary.create over dvs_voc_train (csrc/bow_train.hip).  No CPU fallback:
creating a vocabulary needs the device."""
import ctypes as C
import numpy as np
from ._lib import lib, check, ptr, VocTrainParams, VocTrainReport

L1_NORM = 0
TF_IDF, TF, IDF, BINARY = 0, 1, 2, 3


def _rows(features):
    return np.ascontiguousarray(features, np.uint8).reshape(-1, 32)


class OrbVocabulary:
    """OrbVocabulary: OrbVocabulary(path) / loadFromTextFile, from_arrays(k, L, parent, is_leaf, desc, weight), or create(training
    features, k, L); size(), empty(), transform(), arrays(), save_text().  stream: raw hipStream_t (int) to enqueue on; None = HIP's
    default stream (the handle creates none)."""

    def __init__(self, path=None, device=0, stream=None):
        self._L = lib()
        self._h = None
        self.train_report = None          # dict of dvs_voc_train_report after create() / create_device()
        self._device, self._stream = device, stream
        if path is not None:
            self.loadFromTextFile(path)

    @classmethod
    def from_arrays(cls, k, L, parent, is_leaf, desc, weight, scoring=L1_NORM, weighting=TF_IDF, device=0, stream=None):
        v = cls(None, device, stream)
        parent = np.ascontiguousarray(parent, np.int32).reshape(-1)
        is_leaf = np.ascontiguousarray(is_leaf, np.uint8).reshape(-1)
        desc = _rows(desc); weight = np.ascontiguousarray(weight, np.float64).reshape(-1)
        assert len(parent) == len(is_leaf) == len(desc) == len(weight)
        h = C.c_void_p()
        check(v._L.dvs_bow_vocab_from_arrays(device, stream, k, L, scoring, weighting, len(parent), ptr(parent), ptr(is_leaf), ptr(desc), ptr(weight),
                                             C.byref(h)))
        v._h = h
        return v

    def _train_params(self, k, L, weighting, seed, max_iterations, scoring):
        return VocTrainParams(int(k), int(L), int(weighting), int(scoring), int(seed) & 0xFFFFFFFFFFFFFFFF, int(max_iterations))

    def _trained(self, h, rep):
        self.close()
        self._h = h
        self.train_report = {n: getattr(rep, n) for n, _ in VocTrainReport._fields_}
        return self

    def create(self, training_features, k=10, L=5, weighting=TF_IDF, seed=0, max_iterations=100, scoring=L1_NORM):
        """OrbVocabulary::create(training_features, k, L): training_features is a list of (n_i, 32) uint8 arrays, one per image.
        Replaces this vocabulary (a database that borrows the old one must be gone).  Blocks: the stream is synchronised."""
        images = [_rows(f) for f in training_features]
        counts = np.array([len(f) for f in images], np.int32)
        desc = np.ascontiguousarray(np.concatenate(images)) if images else np.zeros((0, 32), np.uint8)
        prm = self._train_params(k, L, weighting, seed, max_iterations, scoring)
        h, rep = C.c_void_p(), VocTrainReport()
        check(self._L.dvs_voc_train(self._device, self._stream, C.byref(prm), ptr(desc) if len(desc) else None, ptr(counts) if len(counts) else None,
                                    len(counts), C.byref(h), C.byref(rep)))
        return self._trained(h, rep)

    def create_device(self, d_desc, d_n, stride_rows, nframes, k=10, L=5, weighting=TF_IDF, seed=0, max_iterations=100, scoring=L1_NORM):
        """the same on device-resident frames in the layout of transform_batch_device (frame f: rows [0, d_n[f]) of d_desc + f*stride_rows*32)"""
        prm = self._train_params(k, L, weighting, seed, max_iterations, scoring)
        h, rep = C.c_void_p(), VocTrainReport()
        check(self._L.dvs_voc_train_device(self._device, self._stream, C.byref(prm), d_desc, d_n, stride_rows, nframes, C.byref(h), C.byref(rep)))
        return self._trained(h, rep)

    def arrays(self):
        """dict: parent int32[n], is_leaf uint8[n], desc uint8[n, 32], weight float64[n] — what from_arrays takes (row j: node j + 1)"""
        n = self.info()["n_nodes"] if self._h else 0
        parent = np.zeros(n, np.int32); is_leaf = np.zeros(n, np.uint8); desc = np.zeros((n, 32), np.uint8); weight = np.zeros(n, np.float64)
        got = C.c_int32()
        if self._h:
            check(self._L.dvs_voc_get_arrays(self._h, n, ptr(parent), ptr(is_leaf), ptr(desc), ptr(weight), C.byref(got)))
        return dict(parent=parent, is_leaf=is_leaf, desc=desc, weight=weight)

    def save_text(self, path):
        """TemplatedVocabulary::saveToTextFile, the format loadFromTextFile reads"""
        check(self._L.dvs_voc_save_text(self._h, str(path).encode()))

    saveToTextFile = save_text

    def loadFromTextFile(self, path):
        self.close()
        h = C.c_void_p()
        check(self._L.dvs_bow_vocab_load_text(self._device, self._stream, str(path).encode(), C.byref(h)))
        self._h = h
        return True

    def close(self):
        if getattr(self, "_h", None):
            self._L.dvs_bow_vocab_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self):
        v = [C.c_int32() for _ in range(6)]
        check(self._L.dvs_bow_vocab_info(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("k", "L", "scoring", "weighting", "n_nodes", "n_words"), (x.value for x in v)))

    def size(self):
        return self.info()["n_words"] if self._h else 0

    def empty(self):
        return self.size() == 0

    def synchronize(self):
        check(self._L.dvs_bow_vocab_synchronize(self._h))

    def transform(self, features, levelsup=0):
        """dict: words int32[nw] (ascending), values float64[nw], fv_nodes int32[nn] (ascending), fv_offsets int32[nn + 1], fv_features
        int32[fv_offsets[-1]], and per feature feat_word, feat_node int32[n], feat_weight float64[n]"""
        f = _rows(features)
        n = len(f)
        words = np.zeros(n, np.int32); values = np.zeros(n, np.float64)
        fvn = np.zeros(n, np.int32); fvo = np.zeros(n + 1, np.int32); fvf = np.zeros(n, np.int32)
        fw = np.zeros(n, np.int32); fn = np.zeros(n, np.int32); fwt = np.zeros(n, np.float64)
        nw, nn = C.c_int32(), C.c_int32()
        check(self._L.dvs_bow_transform(self._h, ptr(f), n, levelsup, ptr(words), ptr(values), n, C.byref(nw), ptr(fvn), ptr(fvo), ptr(fvf), n, C.byref(nn),
                                        ptr(fw), ptr(fn), ptr(fwt)))
        nw, nn = nw.value, nn.value
        fvo = fvo[:nn + 1].copy()
        return dict(words=words[:nw].copy(), values=values[:nw].copy(), fv_nodes=fvn[:nn].copy(), fv_offsets=fvo, fv_features=fvf[:int(fvo[-1])].copy(),
                    feat_word=fw, feat_node=fn, feat_weight=fwt)

    def transform_batch_device(self, d_desc, d_n, stride_rows, nframes, levelsup, d_word_ids=None, d_word_values=None, d_n_words=None, d_fv_nodes=None,
                               d_fv_offsets=None, d_fv_features=None, d_n_fv_nodes=None, d_feat_word=None, d_feat_node=None, d_feat_weight=None):
        check(self._L.dvs_bow_transform_batch_device(self._h, d_desc, d_n, stride_rows, nframes, levelsup, d_word_ids, d_word_values, d_n_words, d_fv_nodes,
                                                     d_fv_offsets, d_fv_features, d_n_fv_nodes, d_feat_word, d_feat_node, d_feat_weight))


class OrbDatabase:
    """OrbDatabase(vocabulary): add(features) -> entry id, query(features, max_results, max_id) -> [(Id, Score)], size(), clear()"""

    def __init__(self, vocabulary):
        self._voc = vocabulary            # the handle borrows the vocabulary: keep it alive
        self._L = vocabulary._L
        h = C.c_void_p()
        check(self._L.dvs_bow_db_create(vocabulary._h, C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._L.dvs_bow_db_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def size(self):
        return self._L.dvs_bow_db_size(self._h)

    def clear(self):
        check(self._L.dvs_bow_db_clear(self._h))

    def add(self, features):
        f = _rows(features)
        e = C.c_int32(-1)
        check(self._L.dvs_bow_db_add(self._h, ptr(f), len(f), C.byref(e)))
        return e.value

    def add_device(self, d_desc, d_n, stride_rows, nframes):
        e = C.c_int32(-1)
        check(self._L.dvs_bow_db_add_device(self._h, d_desc, d_n, stride_rows, nframes, C.byref(e)))
        return e.value

    def query_arrays(self, features, max_results=0, max_id=-1):
        """(ids int32[], scores float64[])"""
        f = _rows(features)
        size = self.size()
        cap = size if max_results <= 0 else min(max_results, size)
        ids = np.zeros(max(cap, 1), np.int32); scores = np.zeros(max(cap, 1), np.float64)
        n = C.c_int32()
        check(self._L.dvs_bow_db_query(self._h, ptr(f), len(f), max_results, max_id, ptr(ids), ptr(scores), cap, C.byref(n)))
        return ids[:n.value].copy(), scores[:n.value].copy()

    def query(self, features, max_results=0, max_id=-1):
        ids, scores = self.query_arrays(features, max_results, max_id)
        return [(int(i), float(s)) for i, s in zip(ids, scores)]

    def query_device(self, d_desc, d_n, stride_rows, max_results, max_id, d_ids, d_scores, cap, d_n_results):
        check(self._L.dvs_bow_db_query_device(self._h, d_desc, d_n, stride_rows, max_results, max_id, d_ids, d_scores, cap, d_n_results))

    def get_entry(self, entry_id):
        n = C.c_int32()
        code = self._L.dvs_bow_db_get_entry(self._h, entry_id, None, None, 0, C.byref(n))
        if code not in (0, -3):
            check(code)
        words = np.zeros(max(n.value, 1), np.int32); values = np.zeros(max(n.value, 1), np.float64)
        check(self._L.dvs_bow_db_get_entry(self._h, entry_id, ptr(words), ptr(values), n.value, C.byref(n)))
        return words[:n.value].copy(), values[:n.value].copy()
