"""Place recognition on the GPU (csrc/bow.hip) against the sequential restatement tests/bow_ref.py: every comparison is bit for bit —
integers, or doubles produced by the same IEEE operations in the same order (tobytes() equality).  No tolerance anywhere."""
import functools
import numpy as np
import pytest

import bow_ref as br

pytestmark = pytest.mark.gpu
NS = (0, 1, 15, 16, 17, 63, 64, 65, 500)


def f64(values):
    return np.asarray(values, np.float64).tobytes()


@functools.lru_cache(maxsize=None)
def _voc(seed, k, L, weighting=br.TF_IDF):
    return br.make_vocabulary(seed, k, L, weighting)


def _gpu_voc(voc):
    from dvslam_amd import OrbVocabulary
    return OrbVocabulary.from_arrays(voc.k, voc.L, voc.parent, voc.is_leaf, voc.desc, voc.weight, voc.scoring, voc.weighting)


def _check(out, ref):
    words, values, fv, per = ref
    assert out["feat_word"].tolist() == [p[0] for p in per] and out["feat_node"].tolist() == [p[1] for p in per]
    assert out["feat_weight"].tobytes() == f64([p[2] for p in per])
    assert out["words"].tolist() == words and out["values"].tobytes() == f64(values)
    assert out["fv_nodes"].tolist() == [n for n, _ in fv]
    assert out["fv_offsets"].tolist() == np.concatenate([[0], np.cumsum([len(i) for _, i in fv])]).astype(int).tolist()
    assert out["fv_features"].tolist() == [i for _, idx in fv for i in idx]


@pytest.mark.parametrize("k,L", [(2, 1), (3, 3), (10, 3), (17, 2), (32, 2)])
def test_descent_parity(gpu, k, L):
    """per-feature word and node, every planted edge case on: ties (first child wins), fewer than k children, early leaves (their own
    node), weight-0 words; one and two trips over the children (k <= 16, k > 16); feature counts around the 16 features of a block"""
    voc = _voc(21 + k, k, L)
    g = _gpu_voc(voc)
    assert g.info() == dict(k=k, L=L, scoring=0, weighting=0, n_nodes=voc.n_nodes, n_words=voc.n_words) and g.size() == voc.n_words and not g.empty()
    ties = []
    for n in NS:
        feats = br.make_features(voc, 1000 + n, n)
        for levelsup in sorted({0, 1, L - 1, L, L + 2}):
            _check(g.transform(feats, levelsup), br.transform(voc, feats, levelsup))
        for f in feats:
            br.transform_feature(voc, f, 0, ties)
    assert ties, "no feature met two children at the same distance"
    g.close()


@pytest.mark.parametrize("weighting", [br.TF_IDF, br.TF, br.IDF, br.BINARY])
def test_transform_parity_all_weightings(gpu, weighting):
    for k, L, n in ((10, 3, 300), (3, 3, 65)):
        voc = _voc(5, k, L, weighting)
        feats = br.make_features(voc, 77, n)
        ref = br.transform(voc, feats, 1)
        counts = {}
        for word, _, w in ref[3]:
            if w > 0:
                counts[word] = counts.get(word, 0) + 1
        assert max(counts.values()) >= 3, "a word must be counted three times for the addition order to show"
        assert any(w == 0.0 for _, _, w in ref[3]), "a feature must land on a weight-0 word"
        g = _gpu_voc(voc)
        _check(g.transform(feats, 1), ref)
        g.close()


def test_all_weights_zero_and_empty_vocabulary(gpu):
    voc = _voc(5, 10, 3)
    zero = br.Vocabulary(voc.k, voc.L, 0, 0, voc.parent, voc.is_leaf, voc.desc, np.zeros(voc.n_nodes))
    feats = br.make_features(voc, 3, 40)
    g = _gpu_voc(zero)
    out = g.transform(feats)
    _check(out, br.transform(zero, feats))
    assert len(out["words"]) == 0 and len(out["fv_nodes"]) == 0 and out["fv_offsets"].tolist() == [0]
    g.close()
    empty = br.Vocabulary(10, 3, 0, 0, [], [], np.zeros((0, 32), np.uint8), [])
    g = _gpu_voc(empty)
    assert g.empty() and g.size() == 0
    _check(g.transform(feats), br.transform(empty, feats))
    g.close()


def test_batch_device_equals_per_frame_host_calls(gpu):
    from dvslam_amd._lib import DeviceBuffer
    voc = _voc(5, 10, 3)
    g = _gpu_voc(voc)
    stride, counts = 70, [70, 0, 33]
    frames = [br.make_features(voc, 50 + f, stride) for f in range(3)]
    d_desc = DeviceBuffer(3 * stride * 32).upload(np.stack(frames))
    d_n = DeviceBuffer(12).upload(np.array(counts, np.int32))
    i32 = {k: DeviceBuffer(3 * (stride + 1) * 4) for k in ("words", "fv_nodes", "fv_offsets", "fv_features", "feat_word", "feat_node")}
    f8 = {k: DeviceBuffer(3 * stride * 8) for k in ("values", "feat_weight")}
    d_nw, d_nn = DeviceBuffer(12), DeviceBuffer(12)
    g.transform_batch_device(d_desc.ptr, d_n.ptr, stride, 3, 1, i32["words"].ptr, f8["values"].ptr, d_nw.ptr, i32["fv_nodes"].ptr, i32["fv_offsets"].ptr,
                             i32["fv_features"].ptr, d_nn.ptr, i32["feat_word"].ptr, i32["feat_node"].ptr, f8["feat_weight"].ptr)
    g.synchronize()
    nw, nn = d_nw.download(np.int32, 3), d_nn.download(np.int32, 3)
    got_i = {k: b.download(np.int32, 3 * stride).reshape(3, stride) for k, b in i32.items() if k != "fv_offsets"}
    offs = i32["fv_offsets"].download(np.int32, 3 * (stride + 1)).reshape(3, stride + 1)
    got_f = {k: b.download(np.float64, 3 * stride).reshape(3, stride) for k, b in f8.items()}
    for f, n in enumerate(counts):
        one = g.transform(frames[f][:n], 1)
        _check(one, br.transform(voc, frames[f][:n], 1))
        assert nw[f] == len(one["words"]) and nn[f] == len(one["fv_nodes"])
        assert got_i["words"][f, :nw[f]].tolist() == one["words"].tolist() and got_f["values"][f, :nw[f]].tobytes() == one["values"].tobytes()
        assert got_i["fv_nodes"][f, :nn[f]].tolist() == one["fv_nodes"].tolist() and offs[f, :nn[f] + 1].tolist() == one["fv_offsets"].tolist()
        assert got_i["fv_features"][f, :offs[f, nn[f]]].tolist() == one["fv_features"].tolist()
        assert got_i["feat_word"][f, :n].tolist() == one["feat_word"].tolist() and got_i["feat_node"][f, :n].tolist() == one["feat_node"].tolist()
        assert got_f["feat_weight"][f, :n].tobytes() == one["feat_weight"].tobytes()
    # outputs are optional: a call without any leaves the handle's own blocks
    g.transform_batch_device(d_desc.ptr, d_n.ptr, stride, 3, 0)
    g.synchronize()
    g.close()


NQ, M_MAX = 60, 300


@functools.lru_cache(maxsize=None)
def _scene():
    """the query frame and M_MAX entry frames that share 0 %, 10 %, ... 100 % of its descriptors; entry 1 shares no word at all"""
    voc = _voc(5, 10, 3)
    q = br.make_features(voc, 900, NQ)
    q_words = set(br.transform(voc, q)[0])
    pool = br.make_features(voc, 901, 600, random_share=0.5)
    apart = np.stack([f for f in pool if br.transform_feature(voc, f)[0] not in q_words][:NQ])
    assert len(apart) == NQ
    frames = []
    for e in range(M_MAX):
        own = br.make_features(voc, 3000 + e, NQ)
        share = (e % 11) * NQ // 10 if e <= 10 else min((e % 11) * NQ // 10, NQ - 1 - 2 * (e // 11))    # entry 10 alone repeats the whole query
        frames.append(np.concatenate([q[:share], own[share:]]) if e != 1 else apart)
    ref = br.Database(voc)
    for f in frames:
        ref.add(f)
    raws = ref.raw(q)
    assert len({r for r, _ in raws}) == len(raws), "the reference sees an exact tie in raw: choose other inputs"
    assert 1 not in {e for _, e in raws} and len(raws) > M_MAX // 2
    return voc, q, frames, ref


def test_database_add_query_parity(gpu):
    from dvslam_amd import OrbDatabase
    from dvslam_amd._lib import DeviceBuffer
    voc, q, frames, ref = _scene()
    g = _gpu_voc(voc)
    db = OrbDatabase(g)
    assert db.size() == 0 and db.query(q, 0) == []
    d_desc = DeviceBuffer(21 * NQ * 32)
    d_n = DeviceBuffer(21 * 4).upload(np.full(21, NQ, np.int32))
    added = 0
    for M in (1, 2, 65, 300):
        while added < M:
            if 2 <= added and added + 21 <= min(M, 65):            # entries 2 .. 64: three device-resident batches of 21 frames
                d_desc.upload(np.stack(frames[added:added + 21]))
                assert db.add_device(d_desc.ptr, d_n.ptr, NQ, 21) == added
                added += 21
            else:
                assert db.add(frames[added]) == added
                added += 1
        assert db.size() == M
        part = br.Database(voc)
        part.entries = ref.entries[:M]
        for max_results in (0, 1, 5, M + 3):
            for max_id in (-1, 0, 1, M // 2):
                want = part.query(q, max_results, max_id)
                ids, scores = db.query_arrays(q, max_results, max_id)
                assert ids.tolist() == [e for e, _ in want] and scores.tobytes() == f64([s for _, s in want]), (M, max_results, max_id)
        if M >= 2:
            assert 1 not in db.query_arrays(q, 0)[0].tolist(), "an entry without a common word must not appear"
    for e in (0, 1, 2, 30, 64, 65, 299):                            # host adds, device adds, the entry without a common word
        words, values, _, _ = br.transform(voc, frames[e])
        gw, gv = db.get_entry(e)
        assert gw.tolist() == words and gv.tobytes() == f64(values)
        out = g.transform(frames[e])
        assert gw.tolist() == out["words"].tolist() and gv.tobytes() == out["values"].tobytes()
    # the device-rows form
    want = ref.query(q, 7, 200)
    d_q = DeviceBuffer(NQ * 32).upload(q); d_qn = DeviceBuffer(4).upload(np.array([NQ], np.int32))
    d_ids, d_scores, d_nr = DeviceBuffer(7 * 4), DeviceBuffer(7 * 8), DeviceBuffer(4)
    db.query_device(d_q.ptr, d_qn.ptr, NQ, 7, 200, d_ids.ptr, d_scores.ptr, 7, d_nr.ptr)
    g.synchronize()
    assert d_nr.download(np.int32, 1)[0] == 7 and d_ids.download(np.int32, 7).tolist() == [e for e, _ in want]
    assert d_scores.download(np.float64, 7).tobytes() == f64([s for _, s in want])
    # capacity is decided before anything runs
    n = __import__("ctypes").c_int32()
    ids = np.zeros(4, np.int32); sc = np.zeros(4, np.float64)
    assert db._L.dvs_bow_db_query(db._h, q.ctypes.data, NQ, 5, -1, ids.ctypes.data, sc.ctypes.data, 4, __import__("ctypes").byref(n)) == -3
    # clear resets the ids
    db.clear()
    assert db.size() == 0 and db.query(q, 0) == [] and db.add(frames[5]) == 0
    assert db.query(frames[5], 1) == br_query_one(voc, frames[5])
    db.close(); g.close()


def br_query_one(voc, feats):
    d = br.Database(voc)
    d.add(feats)
    return d.query(feats, 1)


def test_identical_entries_come_back_in_ascending_id(gpu):
    from dvslam_amd import OrbDatabase
    voc, q, frames, _ = _scene()
    g = _gpu_voc(voc)
    db = OrbDatabase(g)
    ref = br.Database(voc)
    for f in (frames[3], frames[10], frames[7], frames[10], frames[10]):
        assert db.add(f) == ref.add(f)
    want = ref.query(q, 0)
    assert [e for e, _ in want][:3] == [1, 3, 4] and len({s for _, s in want[:3]}) == 1      # frames[10] shares all of q: the best, three times
    ids, scores = db.query_arrays(q, 0)
    assert ids.tolist() == [e for e, _ in want] and scores.tobytes() == f64([s for _, s in want])
    assert db.query(q, 2) == want[:2]
    db.close(); g.close()


def test_long_query_reads_its_words_from_memory(gpu):
    """more than 4096 query rows: the query's words no longer fit the kernel's LDS block and are searched in memory"""
    from dvslam_amd import OrbDatabase
    voc, q, frames, _ = _scene()
    g = _gpu_voc(voc)
    db = OrbDatabase(g)
    ref = br.Database(voc)
    for f in frames[:6]:
        assert db.add(f) == ref.add(f)
    long_q = np.concatenate([q, br.make_features(voc, 4242, 4200 - NQ)])
    want = ref.query(long_q, 0)
    assert len({s for _, s in want}) == len(want) >= 5
    ids, scores = db.query_arrays(long_q, 0)
    assert ids.tolist() == [e for e, _ in want] and scores.tobytes() == f64([s for _, s in want])
    _check(g.transform(long_q, 1), br.transform(voc, long_q, 1))
    db.close(); g.close()


def test_basic_database_operations_of_the_reference_test(gpu, tmp_path):
    """test_dbow2_integration.cpp:63-126 on the three-disc image, cv::ORB::create(100) descriptors and a (10, 3) vocabulary from a text file"""
    from dvslam_amd import CvORB, OrbVocabulary, OrbDatabase
    from test_oracle_cvorb import disc_image
    orb = CvORB.create(100)
    _, descriptors = orb.detectAndCompute(disc_image())
    orb.close()
    assert len(descriptors) > 0 and descriptors.shape[1] == 32
    voc = br.make_vocabulary(8, 10, 3)
    path = tmp_path / "ORBvoc.txt"
    br.write_text(voc, path)
    vocabulary = OrbVocabulary()
    assert vocabulary.loadFromTextFile(path) and vocabulary.size() == voc.n_words > 0
    _check(vocabulary.transform(descriptors, 2), br.transform(br.parse_text(path), descriptors, 2))
    database = OrbDatabase(vocabulary)
    entry_id = database.add(descriptors)
    assert entry_id >= 0
    results = database.query(descriptors, 1)
    assert len(results) == 1 and results[0][0] == entry_id and results[0][1] > 0.0
    assert f64([results[0][1]]) == f64([br_query_one(voc, descriptors)[0][1]])
    database.close(); vocabulary.close()


def test_unsupported_scoring_in_the_text_header(gpu, tmp_path):
    from dvslam_amd import DvsError, OrbVocabulary
    for scoring in (1, 5):
        voc = br.make_vocabulary(8, 3, 2, scoring=scoring)
        path = tmp_path / f"voc{scoring}.txt"
        br.write_text(voc, path)
        v = OrbVocabulary()
        with pytest.raises(DvsError) as e:
            v.loadFromTextFile(path)
        assert e.value.code == -2 and "L1_NORM" in str(e.value) and v._h is None and v.size() == 0
