"""Loop candidates on the GPU (csrc/loop.hip) against the sequential restatement tests/loop_ref.py: integers and score bytes, bit for
bit.  Every result also goes through the property check: no entry feature matched twice within a candidate, and n_matches equal to the
number of rows with train_idx >= 0."""
import functools
import numpy as np
import pytest

import bow_ref as br
import loop_ref as lr

pytestmark = pytest.mark.gpu
NONE = lr.INT32_MAX


def f64(values):
    return np.asarray(values, np.float64).tobytes()


def _gpu_voc(voc):
    from dvslam_amd import OrbVocabulary
    return OrbVocabulary.from_arrays(voc.k, voc.L, voc.parent, voc.is_leaf, voc.desc, voc.weight, voc.scoring, voc.weighting)


def _props(train, dist, nm):
    train, dist, nm = np.asarray(train), np.asarray(dist), np.asarray(nm)
    for c in range(len(nm)):
        used = train[c][train[c] >= 0]
        assert len(set(used.tolist())) == len(used), "an entry feature is matched twice"
        assert nm[c] == len(used) or (nm[c] == -1 and len(used) == 0)
        assert ((train[c] >= 0) == (dist[c] != NONE)).all()


def _same(got, want):
    _props(*got[:3])
    assert got[2].tolist() == want[2].tolist()
    assert got[0].tolist() == want[0].tolist() and got[1].tolist() == want[1].tolist()


class DeviceMatch:
    """match_device / detect_device with every block allocated here; rows past the query's count are filled with copies of `pad` (rows
    that WOULD match if the kernels looked at them)"""

    def __init__(self, g, db, query, stride, cap, pad=None):
        from dvslam_amd._lib import DeviceBuffer
        self.g, self.db, self.n, self.stride, self.cap = g, db, len(query), stride, cap
        rows = np.zeros((max(stride, 1), 32), np.uint8)
        rows[:len(query)] = query
        if pad is not None and stride > len(query):
            rows[len(query):stride] = pad[:stride - len(query)]
        self.d_q = DeviceBuffer(rows.nbytes).upload(rows)
        self.d_n = DeviceBuffer(4).upload(np.array([len(query)], np.int32))
        c = max(cap, 1)
        self.d_ids, self.d_nc, self.d_scores = DeviceBuffer(c * 4), DeviceBuffer(4), DeviceBuffer(c * 8)
        self.d_train, self.d_dist, self.d_nm = DeviceBuffer(c * max(stride, 1) * 4), DeviceBuffer(c * max(stride, 1) * 4), DeviceBuffer(c * 4)
        for b in (self.d_train, self.d_dist, self.d_nm):           # poison: every slot must be written
            b.upload(np.full(b.nbytes // 4, 7777, np.int32))

    def _out(self):
        self.g.synchronize()
        if self.cap * self.stride == 0:
            train = dist = np.zeros((self.cap, self.stride), np.int32)
        else:
            train = self.d_train.download(np.int32, self.cap * self.stride).reshape(self.cap, self.stride)
            dist = self.d_dist.download(np.int32, self.cap * self.stride).reshape(self.cap, self.stride)
        return train, dist, self.d_nm.download(np.int32, max(self.cap, 1))[:self.cap]

    def match(self, ids, **kw):
        self.d_ids.upload(np.asarray(list(ids) + [0] * (max(self.cap, 1) - len(ids)), np.int32))
        self.d_nc.upload(np.array([len(ids)], np.int32))
        self.db.match_device(self.d_q.ptr, self.d_n.ptr, self.stride, self.d_ids.ptr, self.d_nc.ptr, self.cap, self.d_train.ptr, self.d_dist.ptr,
                             self.d_nm.ptr, **kw)
        return self._out()

    def query_then_match(self, max_results, max_id=-1, **kw):
        self.db.query_device(self.d_q.ptr, self.d_n.ptr, self.stride, max_results, max_id, self.d_ids.ptr, self.d_scores.ptr, self.cap, self.d_nc.ptr)
        self.db.match_device(self.d_q.ptr, self.d_n.ptr, self.stride, self.d_ids.ptr, self.d_nc.ptr, self.cap, self.d_train.ptr, self.d_dist.ptr,
                             self.d_nm.ptr, **kw)
        return self._results()

    def detect(self, max_results, max_id=-1, **kw):
        self.db.detect_device(self.d_q.ptr, self.d_n.ptr, self.stride, max_results, max_id, self.d_ids.ptr, self.d_scores.ptr, self.d_nm.ptr,
                              self.d_train.ptr, self.d_dist.ptr, self.cap, self.d_nc.ptr, **kw)
        return self._results()

    def _results(self):
        train, dist, nm = self._out()
        nr = int(self.d_nc.download(np.int32, 1)[0])
        return self.d_ids.download(np.int32, max(self.cap, 1))[:nr], self.d_scores.download(np.float64, max(self.cap, 1))[:nr], nm, train, dist, nr


def _check_device_rows(got, want, n):
    """device outputs are [cap][stride]: the first len(want) candidates and n rows equal the reference, everything else is unmatched"""
    train, dist, nm = got
    c = len(want[2])
    _props(train, dist, nm)
    assert nm[:c].tolist() == want[2].tolist() and (nm[c:] == 0).all()
    assert train[:c, :n].tolist() == want[0].tolist() and dist[:c, :n].tolist() == want[1].tolist()
    assert (train[:, n:] == -1).all() and (dist[:, n:] == NONE).all() and (train[c:] == -1).all() and (dist[c:] == NONE).all()


@functools.lru_cache(maxsize=None)
def _standard(levels):
    voc, entries, query = lr.standard_scene()
    ref = lr.LoopDatabase(voc, levels)
    for e in entries:
        ref.add(e)
    return voc, entries, query, ref, ref.match(query, [0, 1, 2, 3]), ref.match(query, [3, 1], 64, (9, 10))


@pytest.mark.parametrize("levels", [0, 1, 2, 3])
def test_standard_scene(gpu, levels):
    from dvslam_amd import LoopDatabase
    voc, entries, query, ref, want, want_loose = _standard(levels)
    g = _gpu_voc(voc)
    db = LoopDatabase(g, levels)
    assert db.di_levels() == levels and [db.add(e) for e in entries] == [0, 1, 2, 3] and db.size() == 4
    n = len(query)
    _same(db.match(query, [0, 1, 2, 3]), want)
    _same(db.match(query, [3, 1], 64, (9, 10)), want_loose)
    assert want[2][1] > 120 and want[2][1] > max(want[2][[0, 2, 3]])
    # detect: the query's ids and score bytes, the matches of those ids
    res = ref.inv.query(query, 3)
    order = [e for e, _ in res]
    sub = tuple(np.stack([want[k][e] for e in order]) for k in range(3))
    ids, scores, nm, train, dist = db.detect(query, 3)
    assert ids.tolist() == order and scores.tobytes() == f64([s for _, s in res])
    _same((train, dist, nm), sub)
    ids, scores, nm, train, dist = db.detect(query, 3, max_id=1)        # max_id excludes the later keyframes
    assert ids.tolist() == [0] and scores.tobytes() == f64([s for _, s in ref.inv.query(query, 3, 1)])
    _same((train, dist, nm), tuple(want[k][:1] for k in range(3)))
    # the device forms, the stride longer than the frame and the rows behind it copies of entry 1's (they would match)
    dm = DeviceMatch(g, db, query, n + 37, 5, pad=entries[1])
    _check_device_rows(dm.match([0, 1, 2, 3]), want, n)
    ids, scores, nm, train, dist, nr = dm.query_then_match(3)
    assert nr == 3 and ids.tolist() == order and scores.tobytes() == f64([s for _, s in res])
    _check_device_rows((train, dist, nm), sub, n)
    ids, scores, nm, train, dist, nr = dm.detect(3)
    assert nr == 3 and ids.tolist() == order and scores.tobytes() == f64([s for _, s in res])
    _check_device_rows((train[:3], dist[:3], nm[:3]), sub, n)
    db.close(); g.close()


def test_database_part_equals_orb_database(gpu):
    from dvslam_amd import LoopDatabase, OrbDatabase
    voc, entries, query = lr.standard_scene()
    g = _gpu_voc(voc)
    plain = OrbDatabase(g)
    for levels in (0, 2, 5):
        db = LoopDatabase(g, levels)
        plain.clear()
        for e, rows in enumerate(entries):
            assert db.add(rows) == e == plain.add(rows)
        for max_results, max_id in ((0, -1), (2, -1), (0, 2), (1, 3)):
            a, b = db.query_arrays(query, max_results, max_id), plain.query_arrays(query, max_results, max_id)
            want = br_query(voc, entries, query, max_results, max_id)
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
            assert a[0].tolist() == [e for e, _ in want] and a[1].tobytes() == f64([s for _, s in want])
        assert db.query(query, 1) == plain.query(query, 1)
        for e, rows in enumerate(entries):
            assert db.retrieve_features(e) == br.transform(voc, rows, levels)[2]
            assert db.get_descriptors(e).tobytes() == rows.tobytes()
        db.clear()
        assert db.size() == 0 and db.query(query, 0) == [] and db.add(entries[2]) == 0
        assert db.retrieve_features(0) == br.transform(voc, entries[2], levels)[2] and db.get_descriptors(0).tobytes() == entries[2].tobytes()
        db.close()
    plain.close(); g.close()


def br_query(voc, entries, query, max_results, max_id):
    d = br.Database(voc)
    for e in entries:
        d.add(e)
    return d.query(query, max_results, max_id)


@functools.lru_cache(maxsize=None)
def _segments():
    """one node: entries of 1, 2, 63, 64, 65, 257 rows and of one row more than the kernel's LDS tile; queries of 0, 1, 65 rows and of a
    count that is no multiple of the kernel's query block"""
    from dvslam_amd import loop
    voc = lr.one_node_vocabulary()
    base = lr.random_rows(11, 40)
    sizes = [1, 2, 63, 64, 65, 257, loop.MATCH_TILE_ROWS + 1, 2 * loop.MATCH_TILE_ROWS]
    entries = [lr.near_rows(100 + s, base, s, 30) for s in sizes]
    qsizes = [0, 1, 65, loop.MATCH_QUERY_BLOCK * 2 + 23]
    assert qsizes[-1] % loop.MATCH_QUERY_BLOCK and max(sizes) > loop.MATCH_TILE_ROWS + 1
    queries = [lr.near_rows(200 + s, base, s, 30) for s in qsizes]
    ref = lr.LoopDatabase(voc, voc.L)
    for e in entries:
        ref.add(e)
    ids = list(range(len(sizes)))
    want = [(ref.match(q, ids), ref.match(q, ids, 256, (1, 1))) for q in queries]
    assert any(w[0][2].sum() > 20 for w in want) and all(w[1][2][0] == min(1, len(q)) for w, q in zip(want, queries))
    return voc, entries, queries, ids, want


def test_segment_sizes_on_one_node(gpu):
    """the mirrored constants dvslam_amd.loop.MATCH_TILE_ROWS / MATCH_QUERY_BLOCK are compared with csrc/loop.hip's text by
    tests/test_loop_cpu.py::test_mirrored_kernel_constants: the tile + 1 and two-tile segments below really cross the kernel's tile"""
    from dvslam_amd import LoopDatabase
    voc, entries, queries, ids, want = _segments()
    g = _gpu_voc(voc)
    db = LoopDatabase(g, voc.L)
    for e in entries:
        db.add(e)
    for e, rows in enumerate(entries):
        assert db.retrieve_features(e) == [(0, list(range(len(rows))))]
    for q, (w_default, w_all) in zip(queries, want):
        _same(db.match(q, ids), w_default)
        _same(db.match(q, ids, 256, (1, 1)), w_all)
        dm = DeviceMatch(g, db, q, len(q), len(ids))
        _check_device_rows(dm.match(ids, max_distance=256, ratio=(1, 1)), w_all, len(q))
    db.close(); g.close()


def test_ties(gpu):
    from dvslam_amd import LoopDatabase
    voc = lr.one_node_vocabulary()
    g = _gpu_voc(voc)
    db = LoopDatabase(g, voc.L)
    ref = lr.LoopDatabase(voc, voc.L)
    row = lr.random_rows(5, 1)
    same = np.repeat(row, 9, axis=0)
    near = lr.near_rows(6, row, 20, 25)
    for rows in (same, near):
        assert db.add(rows) == ref.add(rows)
    # an entry of one row repeated: every d1 == d2, nothing passes 3/4; under 1/1 every proposal goes to j = 0 and one query row keeps it
    t, d, nm = db.match(near, [0])
    _same((t, d, nm), ref.match(near, [0]))
    assert nm.tolist() == [0]
    t, d, nm = db.match(near, [0], 256, (1, 1))
    _same((t, d, nm), ref.match(near, [0], 256, (1, 1)))
    assert set(ref.proposals(near, 0, 256, (1, 1)).values()) <= {(0, x) for x in range(257)} and len(ref.proposals(near, 0, 256, (1, 1))) == 20
    assert nm.tolist() == [1] and t[0][t[0] >= 0].tolist() == [0]
    # a query of one row repeated: exactly one match, to i = 0
    t, d, nm = db.match(same, [1], 256, (1, 1))
    _same((t, d, nm), ref.match(same, [1], 256, (1, 1)))
    assert nm.tolist() == [1] and t[0, 0] >= 0 and (t[0, 1:] == -1).all()
    db.close(); g.close()


def test_candidate_lists_and_parameters(gpu):
    from dvslam_amd import LoopDatabase, DvsError
    voc, entries, query, ref, want, _ = _standard(1)
    g = _gpu_voc(voc)
    db = LoopDatabase(g, 1)
    n = len(query)
    # an empty database
    t, d, nm = db.match(query, [])
    assert t.shape == (0, n) and nm.tolist() == []
    with pytest.raises(DvsError) as e:
        db.match(query, [0])
    assert e.value.code == -6
    dm = DeviceMatch(g, db, query, n, 2)
    t, d, nm = dm.match([0])
    assert nm.tolist() == [-1, 0] and (t == -1).all() and (d == NONE).all()
    ids, scores, nm, t, d = db.detect(query, 3)
    assert len(ids) == 0 and t.shape == (0, n)
    assert dm.detect(3)[5] == 0
    # entries: the standard four, then one with 0 rows
    for rows in entries:
        db.add(rows)
    assert db.add(np.zeros((0, 32), np.uint8)) == 4 and db.retrieve_features(4) == [] and len(db.get_descriptors(4)) == 0
    ref5 = lr.LoopDatabase(voc, 1)
    for rows in entries + [np.zeros((0, 32), np.uint8)]:
        ref5.add(rows)
    lists = ([], [1, 1], [4], [4, 2, 4, 1, 0, 3])
    for ids in lists:
        _same(db.match(query, ids), ref5.match(query, ids)[:3])
    # ids out of range: DVS_ERR_ARG in the host form, -1 in the device form; cap_cand larger than the count
    for bad in ([5], [1, -1], [0, 2 ** 31 - 1]):
        with pytest.raises(DvsError) as e:
            db.match(query, bad)
        assert e.value.code == -6
    dm = DeviceMatch(g, db, query, n + 3, 7, pad=entries[1])
    for ids in ([], [1, 1], [2, 5, 1, -1, 4], [0, 1, 2, 3, 4, 1, 99]):
        _check_device_rows(dm.match(ids), ref5.match(query, ids)[:3], n)
    # a query of 0 rows
    empty = np.zeros((0, 32), np.uint8)
    t, d, nm = db.match(empty, [0, 1])
    assert t.shape == (2, 0) and nm.tolist() == [0, 0]
    ids, scores, nm, t, d = db.detect(empty, 2)
    assert len(ids) == 0
    dz = DeviceMatch(g, db, empty, 0, 3)
    assert dz.match([0, 7])[2].tolist() == [0, -1, 0]
    dz = DeviceMatch(g, db, empty, 5, 3, pad=entries[1])              # rows allocated, none valid
    t, d, nm = dz.match([1, 0])
    assert nm.tolist() == [0, 0, 0] and (t == -1).all() and (d == NONE).all()
    # parameters are checked before anything runs
    for md, ratio in ((-1, (3, 4)), (257, (3, 4)), (50, (3, 0)), (50, (3, 32768)), (50, (-1, 4)), (50, (32768, 4))):
        with pytest.raises(DvsError) as e:
            db.match(query, [0], md, ratio)
        assert e.value.code == -6
        with pytest.raises(DvsError) as e:
            db.detect(query, 2, -1, md, ratio)
        assert e.value.code == -6
    _same(db.match(query, [1], 0, (0, 1)), ref5.match(query, [1], 0, (0, 1))[:3])
    _same(db.match(query, [1], 256, (32767, 32767)), ref5.match(query, [1], 256, (32767, 32767))[:3])
    # capacity is decided before anything runs
    import ctypes as C
    nr = C.c_int32()
    a = np.zeros(1, np.int32); s = np.zeros(1, np.float64); big = np.zeros(n, np.int32)
    assert db._L.dvs_loop_db_detect(db._h, query.ctypes.data, n, 3, -1, None, a.ctypes.data, s.ctypes.data, a.ctypes.data, big.ctypes.data, big.ctypes.data,
                                    1, C.byref(nr)) == -3
    db.close(); g.close()


def test_add_device_frames_of_different_lengths(gpu):
    from dvslam_amd import LoopDatabase
    from dvslam_amd._lib import DeviceBuffer
    voc, entries, query = lr.standard_scene()
    g = _gpu_voc(voc)
    stride, counts = 120, [120, 0, 57]
    # the rows behind a frame's count are the query's own rows: they would match at distance 0 if anything looked at them
    frames = [np.concatenate([entries[f][:c], query[:stride - c]]) for f, c in enumerate(counts)]
    d_desc = DeviceBuffer(3 * stride * 32).upload(np.stack(frames))
    d_n = DeviceBuffer(12).upload(np.array(counts, np.int32))
    for levels in (0, 2):
        db = LoopDatabase(g, levels)
        ref = lr.LoopDatabase(voc, levels)
        assert db.add(entries[3][:30]) == ref.add(entries[3][:30]) == 0
        assert db.add_device(d_desc.ptr, d_n.ptr, stride, 3) == 1 and db.size() == 4
        for f, c in enumerate(counts):
            ref.add(frames[f][:c])
        assert db.add(entries[3][30:90]) == ref.add(entries[3][30:90]) == 4
        for e in range(5):
            assert db.get_descriptors(e).tobytes() == ref.rows[e].tobytes() and db.retrieve_features(e) == ref.retrieve_features(e)
        want = ref.match(query, [0, 1, 2, 3, 4], 256, (1, 1))
        got = db.match(query, [0, 1, 2, 3, 4], 256, (1, 1))
        _same(got, want)
        for f, c in enumerate(counts):
            assert (got[0][1 + f] < c).all(), "a row beyond the frame's count was matched"
        assert db.query(query, 0) == ref.query(query, 0)
        db.close()
    g.close()


def test_growth_keeps_the_early_entries(gpu):
    """the per-row blocks start empty and grow to one and a half times what is needed: seven frames of 300 rows make them grow four
    times (450, 900, 1800, 2700+ rows); the per-entry blocks start at 64 entries and 157 entries make them grow twice"""
    from dvslam_amd import LoopDatabase
    voc, entries, query = lr.standard_scene()
    g = _gpu_voc(voc)
    db = LoopDatabase(g, 1)
    ref = lr.LoopDatabase(voc, 1)
    frames = [entries[e % 4] for e in range(7)] + [br.make_features(voc, 500 + e, 4) for e in range(150)]
    for rows in frames:
        assert db.add(rows) == ref.add(rows)
    for e in (0, 1, 2, 5, 6, 7, 70, 156):
        assert db.get_descriptors(e).tobytes() == frames[e].tobytes() and db.retrieve_features(e) == ref.retrieve_features(e)
    ids = [1, 0, 5, 156, 64]
    _same(db.match(query, ids), ref.match(query, ids)[:3])
    got = db.detect(query, 4)
    want = ref.detect(query, 4)
    assert got[0].tolist() == want[0] and got[1].tobytes() == f64(want[1])
    _same((got[3], got[4], got[2]), (want[3], want[4], want[2]))
    db.close(); g.close()
