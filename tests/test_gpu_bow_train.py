"""Vocabulary training on the GPU (csrc/bow_train.hip, OrbVocabulary.create) against the recursive restatement tests/bow_train_ref.py:
every comparison is bit for bit — integers, descriptor bytes, and weights that are glibc's log of the same integer ratio on both sides
(tobytes() equality).  No tolerance anywhere."""
import functools
import numpy as np
import pytest

import bow_ref as br
import bow_train_ref as bt

pytestmark = pytest.mark.gpu
SEED = 11
CASES = [(2, 1, 40), (3, 3, 300), (10, 3, 3000), (17, 2, 700), (32, 2, 2500), (10, 2, 9)]


def f64(values):
    return np.asarray(values, np.float64).tobytes()


@functools.lru_cache(maxsize=None)
def _feats(gen, n):
    f = bt.GENERATORS[gen](SEED, n)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def _tree(gen, k, L, n, seed=0, max_iterations=100):
    return bt.train(_feats(gen, n), k, L, seed, max_iterations)


def _ref(gen, k, L, n, counts, weighting, seed=0, max_iterations=100):
    return bt.weigh(_tree(gen, k, L, n, seed, max_iterations), bt.split(_feats(gen, n), counts), k, L, weighting)


def _same(g, voc, rep):
    a = g.arrays()
    assert g.info() == dict(k=voc.k, L=voc.L, scoring=0, weighting=voc.weighting, n_nodes=voc.n_nodes, n_words=voc.n_words)
    assert a["parent"].tolist() == voc.parent.tolist() and a["is_leaf"].tolist() == voc.is_leaf.tolist()
    assert a["desc"].tobytes() == voc.desc.tobytes()
    assert a["weight"].tobytes() == voc.weight.tobytes()
    assert g.train_report == rep


def _create(images, k, L, weighting=br.TF_IDF, **kw):
    from dvslam_amd import OrbVocabulary
    return OrbVocabulary().create(images, k, L, weighting, **kw)


@pytest.mark.parametrize("gen", ["uniform", "clustered", "dups"])
@pytest.mark.parametrize("k,L,n", CASES)
def test_parity_with_the_restatement(gpu, k, L, n, gen):
    """one image and five unequal images (one of them empty), TF_IDF and TF"""
    assert _tree(gen, k, L, n)[2]["nodes_capped"] == 0, "the cap is a condition of these cases, not a measurement"
    for counts in ([n], bt.five_images(n)):
        for weighting in (br.TF_IDF, br.TF):
            voc, rep = _ref(gen, k, L, n, counts, weighting)
            g = _create(bt.split(_feats(gen, n), counts), k, L, weighting)
            _same(g, voc, rep)
            g.close()


def test_the_matrix_exercises_both_deviations_and_both_paths():
    reports = {(gen, c): _tree(gen, *c)[2] for gen in bt.GENERATORS for c in CASES}
    assert all(r["nodes_capped"] == 0 and r["max_passes"] < 100 for r in reports.values())
    assert any(r["clusters_emptied"] > 0 for r in reports.values()), "no case empties a cluster"
    assert any(r["nodes_short_seeded"] > 0 for r in reports.values()), "no case stops seeding short"
    assert all(reports[("clustered", c)]["clusters_emptied"] > 0 for c in CASES if c[1] > 1 and c[2] > c[0])
    assert all(reports[("dups", c)]["nodes_short_seeded"] > 0 for c in CASES if c[2] > c[0] and c[0] > 3)


@pytest.mark.parametrize("k,L,n", [(3, 2, 0), (3, 2, 1), (3, 2, 3), (3, 2, 4)] +
                         [(k, L, n) for (k, L) in ((3, 2), (17, 1)) for n in (63, 64, 65, 255, 256, 257)])
def test_boundaries(gpu, k, L, n):
    """no feature, one, k, k + 1; totals around the segment and workgroup sizes of the kernels (a node of up to 256 features is a lane
    group's, a larger one is counted by workgroups), k <= 16 and k > 16"""
    counts = bt.five_images(n)
    voc, rep = _ref("uniform", k, L, n, counts, br.TF_IDF)
    g = _create(bt.split(_feats("uniform", n), counts), k, L)
    _same(g, voc, rep)
    assert g.empty() == (n == 0)
    g.close()


def test_root_heavy_node_spans_many_workgroups(gpu):
    k, L, n = 10, 1, 20000
    voc, rep = _ref("uniform", k, L, n, [n], br.TF_IDF)
    g = _create([_feats("uniform", n)], k, L)
    _same(g, voc, rep)
    g.close()


def test_deep_tree_of_many_tiny_nodes(gpu):
    k, L, n = 2, 10, 600
    counts = bt.five_images(n)
    voc, rep = _ref("clustered", k, L, n, counts, br.TF_IDF)
    assert rep["levels_run"] == 10
    g = _create(bt.split(_feats("clustered", n), counts), k, L)
    _same(g, voc, rep)
    g.close()


def test_iteration_cap(gpu):
    k, L, n = 10, 3, 3000
    voc, rep = _ref("uniform", k, L, n, [n], br.TF_IDF, max_iterations=2)
    assert rep["nodes_capped"] > 0 and rep["max_passes"] == 2
    g = _create([_feats("uniform", n)], k, L, max_iterations=2)
    _same(g, voc, rep)
    assert g.train_report["nodes_capped"] > 0
    g.close()


def test_another_seed_is_another_tree_and_still_the_restatement(gpu):
    k, L, n = 3, 3, 300
    voc, rep = _ref("uniform", k, L, n, [n], br.TF_IDF, seed=2 ** 63 + 5)
    assert voc.desc.tobytes() != _ref("uniform", k, L, n, [n], br.TF_IDF)[0].desc.tobytes()
    g = _create([_feats("uniform", n)], k, L, seed=2 ** 63 + 5)
    _same(g, voc, rep)
    g.close()


def _bytes(g):
    a = g.arrays()
    return a["parent"].tobytes() + a["is_leaf"].tobytes() + a["desc"].tobytes() + a["weight"].tobytes()


def test_determinism_and_device_resident_frames(gpu):
    from dvslam_amd import OrbVocabulary
    from dvslam_amd._lib import DeviceBuffer
    k, L, n = 10, 3, 3000
    counts = bt.five_images(n)
    images = bt.split(_feats("clustered", n), counts)
    a = _create(images, k, L)
    b = _create(images, k, L)
    assert _bytes(a) == _bytes(b) and a.train_report == b.train_report
    stride = max(counts) + 37
    block = np.full((len(counts), stride, 32), 0xA5, np.uint8)       # rows past a frame's count are not the frame's
    for f, im in enumerate(images):
        block[f, :len(im)] = im
    d_desc = DeviceBuffer(block.size).upload(block)
    d_n = DeviceBuffer(4 * len(counts)).upload(np.array(counts, np.int32))
    c = OrbVocabulary().create_device(d_desc.ptr, d_n.ptr, stride, len(counts), k, L)
    assert _bytes(c) == _bytes(a) and c.train_report == a.train_report
    _same(c, *_ref("clustered", k, L, n, counts, br.TF_IDF))
    for g in (a, b, c):
        g.close()


def test_trained_vocabulary_in_use(gpu):
    """transform, database add and query on the trained vocabulary equal the restatement's; every image finds itself first"""
    from dvslam_amd import OrbDatabase
    k, L, n = 10, 3, 1500
    counts = [n // 2, n // 5, n // 7, n // 9]
    counts.append(n - sum(counts))
    images = bt.split(_feats("uniform", n), counts)
    voc, rep = _ref("uniform", k, L, n, counts, br.TF_IDF)
    g = _create(images, k, L)
    _same(g, voc, rep)
    db, ref = OrbDatabase(g), br.Database(voc)
    for im in images:
        out = g.transform(im, 1)
        words, values, fv, per = br.transform(voc, im, 1)
        assert out["words"].tolist() == words and out["values"].tobytes() == f64(values)
        assert out["feat_word"].tolist() == [p[0] for p in per] and out["fv_nodes"].tolist() == [x for x, _ in fv]
        assert db.add(im) == ref.add(im)
    for e, im in enumerate(images):
        want = ref.query(im, 0)
        ids, scores = db.query_arrays(im, 0)
        assert ids.tolist() == [i for i, _ in want] and scores.tobytes() == f64([s for _, s in want])
        assert ids[0] == e
    db.close(); g.close()


def test_vocabulary_creation_of_the_reference_test(gpu):
    """test_dbow2_integration.cpp:138-163: cv::ORB::create(100) on the three-disc image, create({descriptors}, 2, 1), size() > 0.  One
    training image: every weight is log(1 / 1) = 0.0"""
    from dvslam_amd import CvORB
    from test_oracle_cvorb import disc_image
    orb = CvORB.create(100)
    _, descriptors = orb.detectAndCompute(disc_image())
    orb.close()
    assert len(descriptors) > 2
    vocabulary = _create([descriptors], 2, 1)
    assert vocabulary.size() > 0
    voc, rep = bt.create([descriptors], 2, 1)
    _same(vocabulary, voc, rep)
    assert vocabulary.arrays()["weight"].tobytes() == f64(np.zeros(voc.n_nodes))
    assert len(vocabulary.transform(descriptors)["words"]) == 0
    vocabulary.close()


def test_save_text_round_trip(gpu, tmp_path):
    from dvslam_amd import OrbVocabulary
    k, L, n = 10, 3, 3000
    counts = bt.five_images(n)
    g = _create(bt.split(_feats("clustered", n), counts), k, L)
    path = tmp_path / "trained.txt"
    g.save_text(path)
    back = OrbVocabulary(path)
    assert _bytes(back) == _bytes(g) and back.info() == g.info()
    assert any(w != 0.0 and w != round(w, 6) for w in g.arrays()["weight"]), "weights that need all 17 digits"
    parsed = br.parse_text(path)
    voc, _ = _ref("clustered", k, L, n, counts, br.TF_IDF)
    assert parsed.parent.tobytes() == voc.parent.tobytes() and parsed.desc.tobytes() == voc.desc.tobytes() and parsed.weight.tobytes() == voc.weight.tobytes()
    back.close(); g.close()
