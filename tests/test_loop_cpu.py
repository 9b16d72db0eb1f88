"""Loop candidates without a GPU: known answers of the restatement (tests/loop_ref.py) worked out by hand, the one-node bracket against
the brute-force k = 2 nearest neighbours of tests/match_modes_ref.py, the standard scene reaching every path of the rule, and the ABI:
dvs_loop_* declared and exported (the set exact), the header compiles as C, the adapter with plain g++ and over the OpenCV stand-ins,
argument errors before any device work, no device means an error."""
import ctypes as C
import os
import re
import subprocess
import numpy as np
import pytest

import bow_ref as br
import loop_ref as lr
import match_modes_ref as mm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["dvs_loop_match_default_params", "dvs_loop_db_create", "dvs_loop_db_destroy", "dvs_loop_db_clear", "dvs_loop_db_size", "dvs_loop_db_di_levels",
           "dvs_loop_db_add", "dvs_loop_db_add_device", "dvs_loop_db_query", "dvs_loop_db_query_device", "dvs_loop_db_get_features",
           "dvs_loop_db_get_descriptors", "dvs_loop_db_match", "dvs_loop_db_match_device", "dvs_loop_db_detect", "dvs_loop_db_detect_device"]
ZERO, ONES = np.zeros(32, np.uint8), np.full(32, 255, np.uint8)
NONE = lr.INT32_MAX


def low(bits, start=0):
    """ZERO with `bits` bits set from bit `start` on: low(a) and low(b) are |a - b| apart, low(a) is a from ZERO"""
    r = ZERO.copy()
    for b in range(start, start + bits):
        r[b >> 3] |= np.uint8(1 << (b & 7))
    return r


def _hand_db(entry, weights=(0.5, 0.25)):
    """k = 2, L = 1: node 1 = word 0 = all zero bits, node 2 = word 1 = all one bits"""
    voc = br.Vocabulary(2, 1, br.L1_NORM, br.TF_IDF, [0, 0], [1, 1], np.stack([ZERO, ONES]), list(weights))
    db = lr.LoopDatabase(voc, 0)
    assert db.add(np.stack(entry)) == 0
    return db


def _one(db, query, max_distance=50, ratio=(3, 4)):
    train, dist, n, cnt = db.match_one(np.stack(query), 0, max_distance, ratio)
    assert n == int((train >= 0).sum())
    return train.tolist(), dist.tolist(), cnt


def test_ratio_inequality_at_equality_and_one_off():
    # d1 * 4 <= d2 * 3: 30, 40 -> 120 <= 120 holds; 31, 40 -> 124 > 120 fails; 30, 41 -> 120 <= 123 holds
    assert _one(_hand_db([low(30), low(40)]), [ZERO])[:2] == ([0], [30])
    t, d, cnt = _one(_hand_db([low(31), low(40)]), [ZERO])
    assert (t, d) == ([-1], [NONE]) and cnt["ratio"] == 1 and cnt["distance"] == 0
    assert _one(_hand_db([low(40), low(30)]), [ZERO])[:2] == ([1], [30])
    assert _one(_hand_db([low(30), low(41)]), [ZERO])[:2] == ([0], [30])
    # other parameters: 1/2 asks for 2 * d1 <= d2
    assert _one(_hand_db([low(20), low(40)]), [ZERO], ratio=(1, 2))[:2] == ([0], [20])
    assert _one(_hand_db([low(21), low(40)]), [ZERO], ratio=(1, 2))[:2] == ([-1], [NONE])


def test_a_lone_entry_feature_has_d2_256():
    t, d, cnt = _one(_hand_db([low(50)]), [ZERO])
    assert (t, d) == ([0], [50]) and cnt["one_member"] == 1          # 50 <= 50 and 200 <= 768
    t, d, cnt = _one(_hand_db([low(51)]), [ZERO])
    assert (t, d) == ([-1], [NONE]) and cnt["distance"] == 1
    # d2 = 256 exactly: with ratio 1/4 a lone feature at 64 passes (64 * 4 <= 256 * 1), at 65 it does not
    assert _one(_hand_db([low(64)]), [ZERO], max_distance=256, ratio=(1, 4))[0] == [0]
    assert _one(_hand_db([low(65)]), [ZERO], max_distance=256, ratio=(1, 4))[0] == [-1]
    # the other node's features do not count: ONES lies under node 2
    assert _one(_hand_db([low(50), ONES]), [ZERO])[:2] == ([0], [50])


def test_the_lowest_j_keeps_a_tie():
    entry = [low(10, 100), low(10), low(10, 50)]                      # all 10 from ZERO
    t, d, cnt = _one(_hand_db(entry), [ZERO])
    assert (t, d) == ([-1], [NONE]) and cnt["d1_eq_d2"] == 1 and cnt["ratio"] == 1      # d1 = d2: 40 > 30
    assert _one(_hand_db(entry), [ZERO], ratio=(1, 1))[:2] == ([0], [10])


def test_conflicts_smaller_d1_then_lower_i():
    db = _hand_db([low(2)])
    t, d, cnt = _one(db, [low(5), low(1)])                            # distances 3 and 1 to the one entry feature
    assert (t, d) == ([-1, 0], [NONE, 1]) and cnt["lost"] == 1
    t, d, cnt = _one(db, [low(3), low(1)])                            # both 1 away: the lower i keeps it
    assert (t, d) == ([0, -1], [1, NONE]) and cnt["lost"] == 1
    t, d, cnt = _one(db, [low(1), low(3), low(2)])                    # 1, 1, 0
    assert (t, d) == ([-1, -1, 0], [NONE, NONE, 0]) and cnt["lost"] == 2


def test_a_weight_0_feature_is_matched_by_nobody():
    db = _hand_db([ZERO, ONES], weights=(0.5, 0.0))
    assert db.retrieve_features(0) == [(1, [0])]
    assert _one(db, [ONES, ZERO])[:2] == ([-1, 0], [NONE, 0])
    assert _one(_hand_db([ZERO, ONES]), [ONES, ZERO])[:2] == ([1, 0], [0, 0])      # with a weight it is


def test_ids_out_of_range_and_repeats():
    db = _hand_db([low(2)])
    train, dist, nm, _ = db.match(np.stack([ZERO]), [0, 5, 0, -1])
    assert nm.tolist() == [1, -1, 1, -1] and train[:, 0].tolist() == [0, -1, 0, -1] and dist[:, 0].tolist() == [2, NONE, 2, NONE]


@pytest.mark.parametrize("params", [(50, (3, 4)), (256, (1, 1)), (40, (1, 2))])
def test_one_root_node_equals_brute_force_knn(params):
    """di_levels >= L and no zero weights: every feature lies under node 0, so the proposals are the two nearest neighbours of a plain
    brute-force matcher put through the same inequality — a second, independent statement of the rule"""
    max_distance, (num, den) = params
    voc = lr.one_node_vocabulary()
    entry = lr.near_rows(1, lr.random_rows(2, 12), 70)
    entry[5] = entry[4]                                               # an exact tie
    query = lr.near_rows(3, entry, 90)
    for levels in (voc.L, voc.L + 2):
        db = lr.LoopDatabase(voc, levels)
        db.add(entry)
        assert db.retrieve_features(0) == [(0, list(range(70)))]
        idx, dist = mm.knn(mm.distances(query, entry), 2)
        want = {}
        for i in range(len(query)):
            d1, d2 = int(dist[i, 0]), (int(dist[i, 1]) if idx[i, 1] >= 0 else 256)
            if d1 <= max_distance and d1 * den <= d2 * num:
                want[i] = (int(idx[i, 0]), d1)
        assert db.proposals(query, 0, max_distance, (num, den)) == want and (len(want) > 5 or max_distance == 40)
    one = lr.LoopDatabase(voc, voc.L)
    one.add(entry[:1])
    idx, dist = mm.knn(mm.distances(query, entry[:1]), 2)
    assert (idx[:, 1] == -1).all()
    assert one.proposals(query, 0, 256, (1, 1)) == {i: (0, int(dist[i, 0])) for i in range(len(query))}


def test_standard_scene_reaches_every_path():
    voc, entries, query = lr.standard_scene()
    for levels in range(4):
        db = lr.LoopDatabase(voc, levels)
        for e in entries:
            db.add(e)
        train, dist, nm, counters = db.match(query, [0, 1, 2, 3])
        assert nm[1] > max(nm[0], nm[2], nm[3]), (levels, nm.tolist())
        assert nm[1] >= 120 and max(nm[0], nm[2], nm[3]) <= 80
        if levels <= 1:
            for name in lr.COUNTERS:
                assert any(c[name] > 0 for c in counters), (levels, name)
        for c in range(4):                                           # one-to-one
            used = train[c][train[c] >= 0]
            assert len(set(used.tolist())) == len(used) == nm[c]
        assert db.query(query, 1)[0][0] == 1


def test_mirrored_kernel_constants():
    from dvslam_amd import loop
    src = open(os.path.join(ROOT, "dynamic-visual-slam_amd", "csrc", "loop.hip")).read()
    assert int(re.search(r"constexpr int kMatchTileRows = (\d+);", src).group(1)) == loop.MATCH_TILE_ROWS
    assert int(re.search(r"constexpr int kMatchQueryBlock = (\d+);", src).group(1)) == loop.MATCH_QUERY_BLOCK


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
    assert sorted(n for n in product if n.startswith("dvs_loop_")) == sorted(SYMBOLS)
    block = header[header.index("loop candidates"):]
    assert "this library's own" in block and "independent of any processing order" in block


def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "loop.c"
    src.write_text('#include "dvslam_hip.h"\nint main(void) { dvs_loop_db* d = 0; dvs_loop_match_params p = {50, 3, 4}; '
                   'return (d || p.max_distance != 50 || p.ratio_num != 3 || p.ratio_den != 4) ? 1 : 0; }\n')
    exe = tmp_path / "loop"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)]).returncode == 0


@pytest.mark.parametrize("opencv", [False, True])
def test_adapter_header_compiles(tmp_path, opencv):
    src = tmp_path / "use.cpp"
    src.write_text('#include "dvslam/loop_detection.hpp"\nint main() { dvslam::LoopDatabase d; dvslam::LoopCandidate c = {0, 0.0, {}}; dvslam::Match m = {0, 0, 0}; '
                   'return (int)d.size() + (int)c.matches.size() + m.query + (d.usingDirectIndex() ? 1 : 0) + d.getDirectIndexLevels() + 1; }\n')
    extra = ["-DDVSLAM_WITH_OPENCV", "-I" + os.path.join(ROOT, "tests", "cpp", "stubs")] if opencv else []
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include")] + extra + [str(src)], check=True)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include")] + extra +
                   [os.path.join(ROOT, "tests", "cpp", "loop_detection_adapter.cpp")], check=True)


def test_argument_errors_come_before_any_device_work(hiplib):
    from dvslam_amd._lib import LoopMatchParams
    L = hiplib
    h, n, m = C.c_void_p(), C.c_int32(), C.c_int32()
    p = LoopMatchParams(1, 1, 1)
    assert L.dvs_loop_match_default_params(None) == -6
    assert L.dvs_loop_match_default_params(C.byref(p)) == 0 and (p.max_distance, p.ratio_num, p.ratio_den) == (50, 3, 4)
    assert L.dvs_loop_db_create(None, 0, C.byref(h)) == -6 and not h.value
    assert L.dvs_loop_db_clear(None) == -6 and L.dvs_loop_db_size(None) == 0 and L.dvs_loop_db_di_levels(None) == -1
    assert L.dvs_loop_db_add(None, None, 0, C.byref(n)) == -6 and L.dvs_loop_db_add_device(None, None, None, 0, 0, C.byref(n)) == -6
    assert L.dvs_loop_db_query(None, None, 0, 1, -1, None, None, 0, C.byref(n)) == -6
    assert L.dvs_loop_db_query_device(None, None, None, 0, 1, -1, None, None, 0, None) == -6
    assert L.dvs_loop_db_get_features(None, 0, None, None, None, 0, 0, C.byref(n), C.byref(m)) == -6
    assert L.dvs_loop_db_get_descriptors(None, 0, None, 0, C.byref(n)) == -6
    assert L.dvs_loop_db_match(None, None, 0, None, 0, C.byref(p), None, None, None) == -6
    assert L.dvs_loop_db_match_device(None, None, None, 0, None, None, 0, C.byref(p), None, None, None) == -6
    assert L.dvs_loop_db_detect(None, None, 0, 1, -1, C.byref(p), None, None, None, None, None, 0, C.byref(n)) == -6
    assert L.dvs_loop_db_detect_device(None, None, None, 0, 1, -1, C.byref(p), None, None, None, None, None, 0, None) == -6
    L.dvs_loop_db_destroy(None)


def test_no_device_means_error_not_fallback(hiplib):
    from dvslam_amd import device_count, DvsError, OrbVocabulary, LoopDatabase
    voc = br.make_vocabulary(1, 2, 1)
    if device_count() > 0:
        v = OrbVocabulary.from_arrays(2, 1, voc.parent, voc.is_leaf, voc.desc, voc.weight)
        db = LoopDatabase(v, 1)
        assert db.size() == 0 and db.di_levels() == 1
        db.close(); v.close()
        return
    with pytest.raises(DvsError) as e:
        LoopDatabase(OrbVocabulary.from_arrays(2, 1, voc.parent, voc.is_leaf, voc.desc, voc.weight), 1)
    assert e.value.code == -5
