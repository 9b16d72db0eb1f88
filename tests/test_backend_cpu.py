"""The mapping backend without a GPU: known answers of the restatement (tests/backend_ref.py) at the edges the kernels must reproduce —
box bounds, first detection wins, the prune rule and its cascade, the id sequences around filtered observations, the window's set order —
and the ABI: dvs_backend_* declared and exported, the header compiles as C, argument errors come before any device work."""
import ctypes as C
import os
import re
import subprocess
import numpy as np
import pytest

import backend_ref as br
from compaction_scenes import crosses_blocks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["dvs_backend_default_params", "dvs_backend_create", "dvs_backend_destroy", "dvs_backend_reset", "dvs_backend_add_keyframe",
           "dvs_backend_add_keyframe_cdr", "dvs_backend_counts", "dvs_backend_get_window", "dvs_backend_apply_optimized", "dvs_backend_prune",
           "dvs_backend_get_landmarks", "dvs_backend_get_observations", "dvs_backend_get_keyframes"]
f32 = np.float32


def test_box_edges_are_inside_one_ulp_outside_is_not():
    det = [(100.0, 50.0, 40.0, 20.0, 4)]                      # x in [80, 120], y in [40, 60]
    for x, y in ((80.0, 50.0), (120.0, 50.0), (100.0, 40.0), (100.0, 60.0), (80.0, 40.0), (120.0, 60.0)):
        assert br.categorize((f32(x), f32(y)), det) == 4, (x, y)
    lo, hi = -np.inf, np.inf
    for x, y in ((np.nextafter(f32(80), f32(lo)), f32(50)), (np.nextafter(f32(120), f32(hi)), f32(50)), (f32(100), np.nextafter(f32(40), f32(lo))),
                 (f32(100), np.nextafter(f32(60), f32(hi)))):
        assert br.categorize((x, y), det) == 0, (x, y)
    # the bounds are computed in double from double fields: a bound that is no float is compared against the promoted pixel
    det = [(100.05, 50.0, 40.0, 20.0, 4)]                     # x in [80.05, 120.05] (doubles)
    assert br.categorize((f32(80.05), f32(50)), det) == (4 if float(f32(80.05)) >= 100.05 - 20.0 else 0)
    assert br.categorize((np.nextafter(f32(80.05), f32(hi)), f32(50)), det) == 4


def test_first_detection_wins_on_overlap():
    det = [(100.0, 100.0, 50.0, 50.0, 2), (110.0, 100.0, 50.0, 50.0, 3)]
    assert br.categorize((f32(105), f32(100)), det) == 2 and br.categorize((f32(105), f32(100)), det[::-1]) == 3
    assert br.categorize((f32(130), f32(100)), det) == 3 and br.categorize((f32(10), f32(10)), det) == 0


def test_prune_rule():
    s = 10**9
    assert not br.prune_rule(1, 5 * s, 25 * s)                 # count 1, age exactly 20.0 s stays
    assert br.prune_rule(1, 5 * s, 25 * s + 1)                 # 20.000000001 s goes
    assert not br.prune_rule(2, 0, 10**6 * s)                  # count 2 stays at any age


def _kf(frame, sec, px, det=(), xyz=None, desc=None):
    n = len(px)
    xyz = np.array(xyz if xyz is not None else [[0.1 * i, 0.0, 3.0] for i in range(n)], np.float64).reshape(-1, 3)
    desc = np.array(desc if desc is not None else [[17 * i + 1] * 32 for i in range(n)], np.uint8).reshape(-1, 32)
    return dict(frame_id=frame, stamp=(sec, 0), translation=(0, 0, 0), rotation_xyzw=br.Q_Z180, landmark_xyz=xyz, obs_pixels=np.array(px, np.float64).reshape(-1, 2),
                obs_desc=desc, detections=list(det))


def test_id_sequences_with_filtered_observations_interleaved():
    ref = br.BackendRef(br.FX, br.FY, br.CX, br.CY, filtered=(1,))
    person = [(50.0, 50.0, 20.0, 20.0, 1)]
    r = ref.add_keyframe(**_kf(0, 0, [(10, 10), (50, 50), (200, 200), (55, 45), (300, 100)], person))
    assert r == dict(n_kept=3, n_filtered=2, n_associated=0, n_created=3, n_moved=0, first_observation_id=0, first_landmark_id=0)
    assert ref.kfs[0]["obs_ids"] == [0, 1, 2] and [o["lm"] for o in ref.obs] == [0, 1, 2]
    assert [tuple(o["px"]) for o in ref.obs] == [(10, 10), (200, 200), (300, 100)]          # ids follow the kept observations only
    r = ref.add_keyframe(**_kf(1, 1, [(50, 50), (400, 400)], person))
    assert (r["first_observation_id"], r["first_landmark_id"], r["n_kept"]) == (3, 3, 1) and ref.next_obs == 4 and ref.next_lm == 4


def test_prune_cascade_counts_and_keyframe_lists():
    ref = br.BackendRef(br.FX, br.FY, br.CX, br.CY)
    X = [[0.2, 0.1, 3.0], [-0.4, 0.3, 3.5], [0.6, -0.2, 2.8]]
    px = [[br.FX * -x / z + br.CX, br.FY * -y / z + br.CY] for x, y, z in X]
    ref.add_keyframe(**_kf(0, 0, px, xyz=X))
    ref.add_keyframe(**_kf(1, 30, px[:1], xyz=X[:1]))          # landmark 0 seen again: count 2
    assert [o["lm"] for o in ref.obs] == [0, 1, 2, 0]
    assert ref.prune((40, 0)) == (2, 2)                         # landmarks 1, 2 (count 1, 40 s old) and their two observations
    assert [o["id"] for o in ref.obs] == [0, 3] and ref.kfs[0]["obs_ids"] == [0] and ref.kfs[1]["obs_ids"] == [3]
    assert sorted(ref.db[0]) == [0] and ref.prune((10**6, 0)) == (0, 0)


def test_the_prune_scene_crosses_the_compaction_blocks():
    """tests/test_gpu_backend.py's prune in the middle: both tables lose rows in several 256-row blocks and keep rows behind them"""
    scene = br.make_scene()
    ref = br.BackendRef(br.FX, br.FY, br.CX, br.CY, filtered=(br.PERSON,))
    for kf in scene[:8]:
        ref.add_keyframe(kf["frame_id"], kf["stamp"], kf["t"], kf["q"], kf["xyz"], kf["px"], kf["desc"], kf["det"])
    lms, obs = ref.landmark_table()["id"], ref.observation_table()["id"]
    assert ref.prune((scene[2]["stamp"][0] + 20, scene[2]["stamp"][1] + 1))[0] > 20
    assert crosses_blocks(lms, ref.landmark_table()["id"]) == (True, True) and crosses_blocks(obs, ref.observation_table()["id"]) == (True, True)


def test_window_is_the_last_five_keyframes_in_set_order():
    ref = br.BackendRef(br.FX, br.FY, br.CX, br.CY)
    for k in range(7):
        ref.add_keyframe(**_kf(10 + k, k, [(30.0 + 40 * k, 100.0), (35.0 + 40 * k, 300.0)], desc=[[k + 1] * 32, [200 - k] * 32]))
    kfs, obs, lms = ref.window()
    assert [k["frame"] for k in kfs] == [12, 13, 14, 15, 16]
    assert [o["id"] for o in obs] == list(range(4, 14)) and [l["id"] for l in lms] == sorted(l["id"] for l in lms) == list(range(4, 14))
    w = ref.window_table()
    assert w["obs_lm_index"].tolist() == list(range(10)) and w["lm_xyz"].dtype == np.float32


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
    assert "typedef struct dvs_backend_params" in header and "typedef struct dvs_detection" in header and "lowest id wins" in header


def test_header_compiles_as_c_and_structs_match_the_mirror(tmp_path):
    from dvslam_amd import backend as B
    src = tmp_path / "sizes.c"
    src.write_text('#include "dvslam_hip.h"\n#include <stdio.h>\nint main(void) { printf("%zu %zu %zu %zu\\n", sizeof(dvs_backend_params), '
                   'sizeof(dvs_detection), sizeof(dvs_backend_result), sizeof(dvs_backend_count)); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    sizes = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert sizes == [C.sizeof(B.BackendParams), C.sizeof(B.Detection), C.sizeof(B.BackendResult), C.sizeof(B.BackendCount)]


def test_adapter_header_compiles(tmp_path):
    src = tmp_path / "use.cpp"
    src.write_text('#include "dvslam/mapping_backend.hpp"\nint main() { return sizeof(dvslam::MappingBackend) > 0 ? 0 : 1; }\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)


def test_defaults_and_argument_errors_without_a_device(hiplib):
    from dvslam_amd import backend as B
    p = B.default_params()
    assert (p.max_descriptor_distance, p.max_reprojection_distance, p.window, p.prune_min_observations, p.prune_max_age_sec, p.n_filtered) == (50.0, 5.0, 5, 2, 20.0, 0)
    L = B._bind(hiplib)
    h = C.c_void_p()
    assert L.dvs_backend_create(None, 0, C.byref(h)) == -6 and L.dvs_backend_create(C.byref(p), 0, C.byref(h)) == -6     # fx = 0
    r = B.BackendResult(); a, b = C.c_int32(), C.c_int32()
    assert L.dvs_backend_add_keyframe(None, None, 0, None, None, None, None, 0, C.byref(r)) == -6
    assert L.dvs_backend_prune(None, 0, 0, C.byref(a), C.byref(b)) == -6 and L.dvs_backend_reset(None) == -6
    with pytest.raises(ValueError):
        B.default_params(filtered_class_ids=range(17))
