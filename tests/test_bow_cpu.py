"""Place recognition without a GPU: known answers of the restatement (tests/bow_ref.py) worked out by hand, the text format through the
restatement's parser and through the library's loader (which parses and checks the file before it asks for a device), and the ABI:
dvs_bow_* declared and exported, the header compiles as C, the adapter header with plain g++, argument errors before any device work."""
import ctypes as C
import os
import re
import subprocess
import numpy as np
import pytest

import bow_ref as br

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["dvs_bow_vocab_load_text", "dvs_bow_vocab_from_arrays", "dvs_bow_vocab_destroy", "dvs_bow_vocab_info", "dvs_bow_vocab_synchronize",
           "dvs_bow_transform", "dvs_bow_transform_batch_device", "dvs_bow_db_create", "dvs_bow_db_destroy", "dvs_bow_db_clear", "dvs_bow_db_size",
           "dvs_bow_db_add", "dvs_bow_db_add_device", "dvs_bow_db_query", "dvs_bow_db_query_device", "dvs_bow_db_get_entry"]
ZERO, ONES = np.zeros(32, np.uint8), np.full(32, 255, np.uint8)


def _hand_vocabulary(weighting=br.TF_IDF):
    """k = 2, L = 1: word 0 = all zero bits, weight 0.5; word 1 = all one bits, weight 0.25"""
    return br.Vocabulary(2, 1, br.L1_NORM, weighting, [0, 0], [1, 1], np.stack([ZERO, ONES]), [0.5, 0.25])


def _hand_features():
    one_bit = ZERO.copy(); one_bit[7] = 0x10
    return np.stack([ZERO, ONES, one_bit])                       # words 0, 1, 0


def test_hand_computed_transform_and_self_query():
    voc = _hand_vocabulary()
    words, values, fv, per = br.transform(voc, _hand_features())
    assert [p[0] for p in per] == [0, 1, 0] and [p[1] for p in per] == [1, 2, 1]
    # v[0] = 0.5 + 0.5 = 1.0, v[1] = 0.25; norm = 1.25; 1.0 / 1.25 and 0.25 / 1.25 correctly rounded are the doubles 0.8 and 0.2
    assert words == [0, 1] and values == [0.8, 0.2]
    assert fv == [(1, [0, 2]), (2, [1])]
    assert br.transform(voc, _hand_features(), levelsup=1)[2] == [(0, [0, 1, 2])]      # L - levelsup = 0: the root
    db = br.Database(voc)
    assert db.add(_hand_features()) == 0
    # raw = (|0.8 - 0.8| - 0.8 - 0.8) + (|0.2 - 0.2| - 0.2 - 0.2) = -fl(1.6) - fl(0.4): the exact sum is 2 + 2^-53, which rounds to 2.0
    assert db.raw(_hand_features()) == [(-2.0, 0)]
    assert db.query(_hand_features(), 1) == [(0, 1.0)]


def test_hand_computed_weightings_and_zero_weight():
    feats = _hand_features()
    assert br.transform(_hand_vocabulary(br.TF), feats)[1] == [0.8, 0.2]
    for w in (br.IDF, br.BINARY):                                # set once: 0.5 and 0.25, norm 0.75
        assert br.transform(_hand_vocabulary(w), feats)[1] == [0.5 / 0.75, 0.25 / 0.75]
    voc = br.Vocabulary(2, 1, 0, 0, [0, 0], [1, 1], np.stack([ZERO, ONES]), [0.5, 0.0])
    words, values, fv, per = br.transform(voc, feats)
    assert words == [0] and values == [1.0] and fv == [(1, [0, 2])] and per[1] == (1, 2, 0.0)   # the weight-0 word contributes nothing
    voc = br.Vocabulary(2, 1, 0, 0, [0, 0], [1, 1], np.stack([ZERO, ONES]), [0.0, 0.0])
    assert br.transform(voc, feats)[:3] == ([], [], [])
    assert br.transform(_hand_vocabulary(), np.zeros((0, 32), np.uint8))[:3] == ([], [], [])


def test_repeated_addition_is_not_a_product():
    """a word seen three times is (w + w) + w: for w = 0.1 that is not 3 * w in doubles... the restatement must keep the order"""
    voc = br.Vocabulary(2, 1, 0, br.TF, [0, 0], [1, 1], np.stack([ZERO, ONES]), [0.1, 0.7])
    feats = np.stack([ZERO, ZERO, ZERO, ONES])
    words, values, _, _ = br.transform(voc, feats)
    a = (0.1 + 0.1) + 0.1
    assert a != 0.3 and values == [a / (a + 0.7), 0.7 / (a + 0.7)]


def test_first_child_wins_ties_and_early_leaves_are_their_own_node():
    b = ZERO.copy(); b[0] = 3                                    # two bits from ZERO
    voc = br.Vocabulary(3, 2, 0, 0, [0, 0, 0, 3, 3], [1, 1, 0, 1, 1], np.stack([ZERO, b, ONES, ONES, ZERO]), [1.0, 2.0, 0.0, 3.0, 4.0])
    probe = ZERO.copy(); probe[0] = 1                            # distance 1 to node 1 (ZERO) and to node 2 (b)
    ties = []
    assert br.transform_feature(voc, probe, 0, ties) == (0, 1, 1.0) and ties == [1]
    # node 1 is a leaf at depth 1 < L = 2: levelsup 0 asks for level 2, which the descent never reaches: the leaf itself
    assert br.transform_feature(voc, ZERO, 0)[1] == 1 and br.transform_feature(voc, ZERO, 1)[1] == 1 and br.transform_feature(voc, ZERO, 2)[1] == 0
    assert br.transform_feature(voc, ONES, 0) == (2, 4, 3.0) and br.transform_feature(voc, ONES, 1) == (2, 3, 3.0)


def test_query_score_is_the_pairwise_l1_score():
    voc = br.make_vocabulary(5, 10, 3)
    db = br.Database(voc)
    frames = [br.make_features(voc, 100 + i, 40) for i in range(4)]
    for f in frames:
        db.add(f)
    q = br.make_features(voc, 100, 40); q[20:] = frames[2][20:]
    qw, qv, _, _ = br.transform(voc, q)
    res = dict(db.query(q, 0))
    assert len(res) >= 2
    for e, score in res.items():
        ew, ev, _, _ = br.transform(voc, frames[e])
        assert score == br.l1_score(qw, qv, ew, ev)
    assert res[0] > 0 and max(res.values()) <= 1.0


def test_builder_plants_the_edge_cases():
    voc = br.make_vocabulary(7, 10, 3)
    nchild = [len(c) for c in voc.children]
    depth = [0] * (voc.n_nodes + 1)
    for nid in range(1, voc.n_nodes + 1):
        depth[nid] = depth[voc.parent[nid - 1]] + 1
    assert any(0 < n < 10 for n in nchild), "nodes with fewer than k children"
    assert any(voc.is_leaf[j] and depth[j + 1] < 3 for j in range(voc.n_nodes)), "leaves above depth L"
    assert any(voc.is_leaf[j] and voc.weight[j] == 0.0 for j in range(voc.n_nodes)), "words of weight 0"
    ties = []
    assert br.transform_feature(voc, br.tie_probe(voc), 0, ties)[0] >= 0 and ties, "the probe ties at the root"
    feats = br.make_features(voc, 3, 50)
    assert (feats[0] == feats[1]).all() and (feats[0] == feats[2]).all()
    assert max(depth) == 3 and any(abs(voc.children[p][i] - voc.children[p][i + 1]) > 1 for p in range(voc.n_nodes + 1) for i in range(len(voc.children[p]) - 1)), \
        "children are not contiguous ids: the loader has to renumber"


def test_text_format_round_trip(tmp_path, hiplib):
    voc = br.make_vocabulary(11, 4, 3)
    path = tmp_path / "voc.txt"
    br.write_text(voc, path)
    back = br.parse_text(path)
    assert (back.k, back.L, back.scoring, back.weighting) == (4, 3, 0, 0)
    assert back.parent.tobytes() == voc.parent.tobytes() and back.is_leaf.tobytes() == voc.is_leaf.tobytes()
    assert back.desc.tobytes() == voc.desc.tobytes() and back.weight.tobytes() == voc.weight.tobytes()
    assert back.children == voc.children and back.word_id == voc.word_id
    # the library's loader parses and checks the file before it touches a device: a good file gets as far as the device
    from dvslam_amd import device_count
    h = C.c_void_p()
    code = hiplib.dvs_bow_vocab_load_text(0, None, str(path).encode(), C.byref(h))
    assert code == (0 if device_count() > 0 else -5)
    if code == 0:
        hiplib.dvs_bow_vocab_destroy(h)


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return set(line.split()[-1] for line in out.splitlines() if line.strip())


def test_symbols_declared_and_exported(hiplib):
    from dvslam_amd import _lib
    header = open(os.path.join(ROOT, "include", "dvslam_hip.h")).read()
    product = _exports(_lib.SO_PATH)
    for s in SYMBOLS:
        assert re.search(r"\b" + s + r"\(", header), s
        assert s in product, s
    assert sorted(n for n in product if n.startswith("dvs_bow_")) == sorted(SYMBOLS)
    assert "PARITY UNPINNED" in header[header.index("place recognition"):] and "test_dbow2_integration.cpp:91" in header


def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "bow.c"
    src.write_text('#include "dvslam_hip.h"\nint main(void) { dvs_bow_vocab* v = 0; dvs_bow_db* d = 0; return (v || d || DVS_BOW_BINARY != 3 || DVS_BOW_MAX_K != 32) ? 1 : 0; }\n')
    exe = tmp_path / "bow"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)]).returncode == 0


def test_adapter_header_compiles(tmp_path):
    src = tmp_path / "use.cpp"
    src.write_text('#include "dvslam/place_recognition.hpp"\nint main() { dvslam::QueryResults r; dvslam::OrbVocabulary v; dvslam::OrbDatabase d; '
                   'return (int)r.size() + (int)v.size() + (int)d.size(); }\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)


def test_argument_errors_come_before_any_device_work(hiplib, tmp_path):
    """bad headers, bad trees and unsupported scorings are told apart on the host: the codes are the same with or without a GPU"""
    L = hiplib
    h = C.c_void_p()
    parent = np.array([0, 0], np.int32); leaf = np.array([1, 1], np.uint8); desc = np.zeros((2, 32), np.uint8); w = np.array([1.0, 2.0])

    def arrays(k=2, depth=1, s=0, wt=0, parent=parent, leaf=leaf, w=w):
        parent = np.ascontiguousarray(parent, np.int32); leaf = np.ascontiguousarray(leaf, np.uint8); w = np.ascontiguousarray(w, np.float64)
        d = np.zeros((len(parent), 32), np.uint8)
        return L.dvs_bow_vocab_from_arrays(0, None, k, depth, s, wt, len(parent), parent.ctypes.data, leaf.ctypes.data, d.ctypes.data, w.ctypes.data, C.byref(h))
    assert arrays(k=1) == -6 and arrays(k=33) == -6 and arrays(depth=0) == -6 and arrays(depth=11) == -6 and arrays(wt=4) == -6 and arrays(s=6) == -6
    for s in (1, 2, 3, 4, 5):
        assert arrays(s=s) == -2 and b"L1_NORM" in L.dvs_last_error() and not h.value
    assert arrays(parent=[0, 2]) == -6 and b"not smaller" in L.dvs_last_error()        # a parent id that is not smaller than the node's own
    assert arrays(parent=[1, 0]) == -6
    assert arrays(leaf=[0, 1]) == -6 and b"no children" in L.dvs_last_error()          # a non-leaf without children
    assert arrays(parent=[0, 1], leaf=[1, 1]) == -6                                     # a leaf with children
    assert arrays(parent=[0, 0, 0], leaf=[1, 1, 1], w=[1, 1, 1]) == -6                  # more than k children
    assert arrays(w=[1.0, np.inf]) == -6
    assert L.dvs_bow_vocab_from_arrays(0, None, 2, 1, 0, 0, 2, None, None, None, None, C.byref(h)) == -6
    assert L.dvs_bow_vocab_load_text(0, None, None, C.byref(h)) == -6
    assert L.dvs_bow_vocab_load_text(0, None, str(tmp_path / "missing.txt").encode(), C.byref(h)) == -6
    for name, text, code in (("short.txt", "10 3 0\n", -6), ("scoring.txt", "2 1 1 0\n0 1 " + "0 " * 32 + "1.0\n", -2),
                             ("fields.txt", "2 1 0 0\n0 1 " + "0 " * 31 + "1.0\n", -6), ("byte.txt", "2 1 0 0\n0 1 " + "256 " * 32 + "1.0\n", -6),
                             ("extra.txt", "2 1 0 0\n0 1 " + "0 " * 32 + "1.0 7\n", -6)):
        p = tmp_path / name
        p.write_text(text)
        assert L.dvs_bow_vocab_load_text(0, None, str(p).encode(), C.byref(h)) == code, name
        assert not h.value
    # NULL handles
    n = C.c_int32()
    assert L.dvs_bow_vocab_info(None, None, None, None, None, None, C.byref(n)) == -6 and L.dvs_bow_vocab_synchronize(None) == -6
    assert L.dvs_bow_transform(None, None, 0, 0, None, None, 0, None, None, None, None, 0, None, None, None, None) == -6
    assert L.dvs_bow_db_create(None, C.byref(h)) == -6 and L.dvs_bow_db_clear(None) == -6 and L.dvs_bow_db_size(None) == 0
    assert L.dvs_bow_db_add(None, None, 0, C.byref(n)) == -6 and L.dvs_bow_db_query(None, None, 0, 1, -1, None, None, 0, C.byref(n)) == -6
    assert L.dvs_bow_db_get_entry(None, 0, None, None, 0, C.byref(n)) == -6
    L.dvs_bow_vocab_destroy(None); L.dvs_bow_db_destroy(None)


def test_no_device_means_error_not_fallback(hiplib):
    from dvslam_amd import device_count, DvsError, OrbVocabulary
    voc = br.make_vocabulary(1, 2, 1)
    if device_count() > 0:
        assert OrbVocabulary.from_arrays(2, 1, voc.parent, voc.is_leaf, voc.desc, voc.weight).size() == 2
        return
    with pytest.raises(DvsError) as e:
        OrbVocabulary.from_arrays(2, 1, voc.parent, voc.is_leaf, voc.desc, voc.weight)
    assert e.value.code == -5
