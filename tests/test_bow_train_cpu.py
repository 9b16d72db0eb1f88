"""Vocabulary training without a GPU: known answers of the restatement (tests/bow_train_ref.py) worked out by hand, the text format
through the restatement's parser, and the ABI: dvs_voc_* declared and exported, the header compiles as C, the adapter with plain g++
(with and without the OpenCV stand-ins), argument errors before any device work."""
import ctypes as C
import math
import os
import re
import subprocess
import numpy as np
import pytest

import bow_ref as br
import bow_train_ref as bt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["dvs_voc_train_default_params", "dvs_voc_train", "dvs_voc_train_device", "dvs_voc_get_arrays", "dvs_voc_save_text"]


def bits(*set_bits):
    """a descriptor with the given bits set (bit b = bit b & 7 of byte b >> 3)"""
    d = np.zeros(32, np.uint8)
    for b in set_bits:
        d[b >> 3] |= np.uint8(1 << (b & 7))
    return d


def test_splitmix64_known_values():
    # the published splitmix64 stream from state 0: its first two outputs
    assert bt.splitmix64(0) == 0xE220A8397B1DCDAF and bt.splitmix64(bt.GOLDEN) == 0x6E789E6AA1B965F4
    assert bt.draw(5, 0) == bt.splitmix64(5) and bt.draw(5, 2) == bt.splitmix64((5 + 2 * bt.GOLDEN) & bt.MASK)


def test_mean_threshold_on_even_and_odd_counts():
    """N/2 + N%2: of 4 rows a bit needs 2, of 5 rows 3, of 1 row 1"""
    rows = np.stack([bits(0, 1, 2), bits(0, 1), bits(0, 9), bits(200)])
    assert bt.mean_value(rows).tobytes() == bits(0, 1).tobytes()                       # counts 3, 2, 1, 1, 1: >= 2 keeps bits 0 and 1
    rows5 = np.concatenate([rows, bits(1, 2, 9)[None]])
    assert bt.mean_value(rows5).tobytes() == bits(0, 1).tobytes()                      # counts 3, 3, 2, 2, 1: >= 3
    assert bt.mean_value(rows5[:1]).tobytes() == rows5[0].tobytes()


def _five():
    """A = 0, B = one bit, C = two bits; D and E near the all-ones row"""
    ones = [b for b in range(256)]
    return np.stack([bits(), bits(0), bits(0, 1), bits(*ones), bits(*ones[1:])])


def test_five_features_k2_worked_by_hand():
    F = _five()
    key = bt.splitmix64(0)
    # seeding: the first centre at u_0 mod 5; min_dist to it; cut = 1 + u_1 mod S; the first inclusive prefix sum >= cut
    first = bt.draw(key, 0) % 5
    dist_to = {0: [0, 1, 2, 256, 255], 1: [1, 0, 1, 255, 254], 2: [2, 1, 0, 254, 253], 3: [256, 255, 254, 0, 1], 4: [255, 254, 253, 1, 0]}
    md = dist_to[first]
    assert bt.distances(F, F[first]).tolist() == md
    S = sum(md)
    cut = 1 + bt.draw(key, 1) % S
    prefix = np.cumsum(md).tolist()
    second = next(i for i, p in enumerate(prefix) if p >= cut)
    assert bt.seed_kmpp(F, 2, key) == [first, second]
    # whichever two seeds: with S dominated by the far group the second seed is in the other group (checked, not assumed)
    assert (first < 3) != (second < 3)
    # pass 1 splits {A, B, C} from {D, E}; pass 2: the means are B (bit 0 in 2 of 3 >= 2, bit 1 in 1 of 3 < 2) and, of two rows with
    # threshold 1, D (bit 0 in 1 of 2 >= 1); the association does not change: two passes
    parent, desc, rep = bt.train(F, 2, 1)
    low, high = (0, 1) if first < 3 else (1, 0)
    assert parent == [0, 0] and desc[low].tobytes() == bits(0).tobytes() and desc[high].tobytes() == F[3].tobytes()
    assert rep["max_passes"] == 2 and rep["nodes_capped"] == 0 and rep["levels_run"] == 1 and rep["clusters_emptied"] == 0
    # with one pass allowed the seeds stay the centres and the node counts as capped
    parent1, desc1, rep1 = bt.train(F, 2, 1, max_iterations=1)
    assert desc1.tobytes() == F[[first, second]].tobytes() and rep1["nodes_capped"] == 1 and rep1["max_passes"] == 1


def test_trivial_case_one_cluster_per_feature_in_order():
    F = _five()[:3]
    for k in (3, 4):
        voc, rep = bt.create([F], k, 2)
        assert voc.parent.tolist() == [0, 0, 0] and voc.is_leaf.tolist() == [1, 1, 1] and voc.desc.tobytes() == F.tobytes()
        assert rep["max_passes"] == 0 and rep["levels_run"] == 1 and rep["n_words"] == 3
    voc, rep = bt.create([], 3, 2)
    assert voc.n_nodes == 0 and voc.n_words == 0 and rep["levels_run"] == 0


def test_duplicates_give_fewer_than_k_children():
    a, b = bits(3), bits(100, 101)
    F = np.stack([a, b, a, a, b, b, a])
    voc, rep = bt.create([F], 4, 1)
    assert voc.n_nodes == 2 and rep["nodes_short_seeded"] == 1
    assert sorted(d.tobytes() for d in voc.desc) == sorted([a.tobytes(), b.tobytes()])
    # all features equal: one child per level, a chain down to L
    voc, rep = bt.create([np.stack([a] * 6)], 3, 3)
    assert voc.parent.tolist() == [0, 1, 2] and voc.is_leaf.tolist() == [0, 0, 1] and rep["nodes_short_seeded"] == 3


def test_node_id_order_on_a_two_level_tree():
    """children have consecutive ids; everything below child 0 precedes everything below child 1"""
    F = bt.clustered(3, 60)
    voc, rep = bt.create([F], 3, 2)
    top = voc.children[0]
    assert top == [1, 2, 3]
    below = [voc.children[c] for c in top]
    assert all(kids == list(range(kids[0], kids[0] + len(kids))) for kids in below if kids)
    flat = [n for kids in below for n in kids]
    assert flat == list(range(4, voc.n_nodes + 1)) and rep["levels_run"] == 2
    assert [voc.word_id[n] for n in range(1, voc.n_nodes + 1) if voc.word_id[n] >= 0] == list(range(voc.n_words))


def test_idf_weights_by_hand():
    a, b, c = bits(), bits(*range(100)), bits(*range(128, 256))
    # four features, k = 4: the trivial case, words 0..3 = a, b, a, c in order.  The descent sends every `a` to word 0 (the first of two
    # equal children), so word 2 is reached by no feature: Ni = [2, 1, 0, 1] over the 3 images
    images = [np.stack([a, b]), np.stack([a]), np.stack([c])]
    voc, _ = bt.create(images, 4, 1, br.TF_IDF)
    assert voc.desc.tobytes() == np.stack([a, b, a, c]).tobytes() and voc.is_leaf.tolist() == [1, 1, 1, 1]
    assert voc.weight.tolist() == [math.log(3.0 / 2.0), math.log(3.0 / 1.0), 0.0, math.log(3.0 / 1.0)]
    assert bt.create(images, 4, 1, br.IDF)[0].weight.tobytes() == voc.weight.tobytes()
    assert bt.create(images, 4, 1, br.TF)[0].weight.tolist() == [1.0] * 4 == bt.create(images, 4, 1, br.BINARY)[0].weight.tolist()
    # an empty image still counts as a document
    assert bt.create(images + [np.zeros((0, 32), np.uint8)], 4, 1)[0].weight.tolist() == [math.log(4.0 / 2.0), math.log(4.0), 0.0, math.log(4.0)]
    # one training image: every weight is log(1 / 1) = 0, and every BowVector is empty
    voc, _ = bt.create([np.concatenate(images)], 4, 1, br.TF_IDF)
    assert voc.n_words == 4 and voc.weight.tolist() == [0.0, 0.0, 0.0, 0.0]
    assert br.transform(voc, images[0])[:3] == ([], [], [])


def test_save_parse_round_trip(tmp_path):
    voc, _ = bt.create(bt.split(bt.clustered(5, 200), bt.five_images(200)), 4, 3)
    assert any(w not in (0.0,) for w in voc.weight)
    path = tmp_path / "trained.txt"
    br.write_text(voc, path)
    back = br.parse_text(path)
    assert back.parent.tobytes() == voc.parent.tobytes() and back.is_leaf.tobytes() == voc.is_leaf.tobytes()
    assert back.desc.tobytes() == voc.desc.tobytes() and back.weight.tobytes() == voc.weight.tobytes()


def test_symbols_declared_and_exported(hiplib):
    from dvslam_amd import _lib
    header = open(os.path.join(ROOT, "include", "dvslam_hip.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.SO_PATH], capture_output=True, text=True, check=True).stdout
    product = set(line.split()[-1] for line in out.splitlines() if line.strip())
    for s in SYMBOLS:
        assert re.search(r"\b" + s + r"\(", header), s
        assert s in product, s
    assert sorted(n for n in product if n.startswith("dvs_voc_")) == sorted(SYMBOLS)
    assert "Not built either: vocabulary.create()" not in header and "vocabulary training" in header


def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "voc.c"
    src.write_text('#include "dvslam_hip.h"\nint main(void) { dvs_voc_train_params p; dvs_voc_train_report r; r.n_nodes = 0; p.seed = 1;\n'
                   '  return (int)(sizeof(p) != 32) + r.n_nodes + (sizeof(r) != 28); }\n')
    exe = tmp_path / "voc"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)]).returncode == 0


@pytest.mark.parametrize("opencv", [False, True])
def test_adapter_compiles(tmp_path, opencv):
    src = tmp_path / "use.cpp"
    body = ('std::vector<dvslam::DescriptorVector> t(1); dvslam::OrbVocabulary v(9, 3, dvslam::TF_IDF, dvslam::L1_NORM), w;\n'
            'if (v.size() == 99) { w.create(t, 2, 1); w.create(t); w.create(t, 2, 1, dvslam::TF, dvslam::L1_NORM); w.saveToTextFile("x"); w.setSeed(3); }\n')
    if opencv:
        body += 'std::vector<std::vector<cv::Mat>> m(1); if (v.size() == 99) { w.create(m, 2, 1); w.create(m); w.create(m, 2, 1, dvslam::TF, dvslam::L1_NORM); }\n'
    src.write_text('#include "dvslam/place_recognition.hpp"\nint main() {\n' + body + 'return (int)v.size() + w.lastTrainReport().n_nodes; }\n')
    extra = ["-DDVSLAM_WITH_OPENCV", "-I" + os.path.join(ROOT, "tests", "cpp", "stubs")] if opencv else []
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include")] + extra + [str(src)], check=True)


def test_argument_errors_come_before_any_device_work(hiplib):
    """the codes are the same with or without a GPU"""
    from dvslam_amd._lib import VocTrainParams, VocTrainReport
    L = hiplib
    h = C.c_void_p()
    desc = np.zeros((4, 32), np.uint8); counts = np.array([3, 1], np.int32)

    def params(**kw):
        p = VocTrainParams()
        assert L.dvs_voc_train_default_params(C.byref(p)) == 0
        for name, value in kw.items():
            setattr(p, name, value)
        return p

    p = params()
    assert (p.k, p.L, p.weighting, p.scoring, p.seed, p.max_iterations) == (10, 5, 0, 0, 0, 100)

    def host(p, desc=desc, counts=counts, n=2):
        return L.dvs_voc_train(0, None, C.byref(p), desc.ctypes.data if desc is not None else None,
                               counts.ctypes.data if counts is not None else None, n, C.byref(h), None)

    def device(p, d_desc=0x1000, d_n=0x1000, stride=4, n=2):
        return L.dvs_voc_train_device(0, None, C.byref(p), d_desc, d_n, stride, n, C.byref(h), None)

    for call in (host, device):
        for bad in (dict(k=1), dict(k=33), dict(L=0), dict(L=11), dict(max_iterations=0), dict(weighting=-1), dict(weighting=4), dict(scoring=6)):
            assert call(params(**bad)) == -6, bad
            assert not h.value
        for s in (1, 2, 3, 4, 5):
            assert call(params(scoring=s)) == -2 and b"L1_NORM" in L.dvs_last_error() and not h.value
    assert host(params(), counts=np.array([3, -1], np.int32)) == -6 and b"negative" in L.dvs_last_error()
    assert host(params(), desc=None) == -6 and host(params(), counts=None) == -6 and host(params(), n=-1) == -6
    assert device(params(), d_desc=None) == -6 and device(params(), d_n=None) == -6 and device(params(), n=-1) == -6 and device(params(), stride=-1) == -6
    assert device(params(), d_desc=0x1008) == -6                                   # rows are read 16 bytes at a time
    assert L.dvs_voc_train(0, None, None, desc.ctypes.data, counts.ctypes.data, 2, C.byref(h), None) == -6
    assert L.dvs_voc_train(0, None, C.byref(params()), desc.ctypes.data, counts.ctypes.data, 2, None, None) == -6
    assert L.dvs_voc_train_default_params(None) == -6
    n = C.c_int32()
    assert L.dvs_voc_get_arrays(None, 0, None, None, None, None, C.byref(n)) == -6 and L.dvs_voc_save_text(None, b"x") == -6
    assert C.sizeof(VocTrainParams) == 32 and C.sizeof(VocTrainReport) == 28


def test_no_device_means_error_not_fallback(hiplib):
    from dvslam_amd import device_count, DvsError, OrbVocabulary
    F = bt.uniform(1, 20)
    if device_count() > 0:
        assert OrbVocabulary().create([F], 2, 1).size() == 2
        return
    with pytest.raises(DvsError) as e:
        OrbVocabulary().create([F], 2, 1)
    assert e.value.code == -5
