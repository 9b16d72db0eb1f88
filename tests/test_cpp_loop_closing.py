"""C++ adapter dvslam::closeLoop (include/dvslam/loop_closing.hpp) and the loop-closing members of dvslam::MappingBackend:
tests/cpp/loop_closing.cpp compiles with g++ -std=c++17 -Wall -Werror against the C-ABI and refuses to run without a GPU (exit code 3); on
the GPU, fed the scene of tests/loop_closing_ref.py from a file, it writes the same text — anchors, pose graph, the result of the close and
the CRC-32 of every table column after the close, after a dry-run fusion and after the applied one — as the Python handle."""
import os
import struct
import subprocess
import zlib
import numpy as np
import pytest

import loop_closing_ref as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "dynamic-visual-slam_amd", "lib")


def _build(tmpdir):
    exe = os.path.join(str(tmpdir), "loop_closing")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "loop_closing.cpp"),
                           "-o", exe, "-L" + LIBDIR, "-ldvslam_hip", "-Wl,-rpath," + LIBDIR, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_adapter_compiles_and_refuses_without_gpu(tmp_path, hiplib):
    from dvslam_amd import device_count
    code = subprocess.call([_build(tmp_path)], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    assert code == (2 if device_count() > 0 else 3)       # with a GPU and no arguments: the usage exit


def _crc(a):
    return "%08x" % (zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xFFFFFFFF)


def _map_text(mb):
    L, O, K = mb.landmarks(), mb.observations(), mb.keyframes()
    lm = " ".join(_crc(L[k]) for k in ("id", "class_id", "xyz", "desc", "observation_count", "last_seen_ns", "obs_offsets", "obs_ids"))
    ob = " ".join(_crc(O[k]) for k in ("id", "frame_id", "px", "desc", "class_id", "landmark_id"))
    kf = " ".join(_crc(K[k]) for k in ("frame_id", "stamp_ns", "R", "t", "obs_offsets", "obs_ids"))
    return f"lm={len(L['id'])} {lm} ob={len(O['id'])} {ob} kf={len(K['frame_id'])} {kf}"


def _fuse_text(tag, f):
    return f"{tag} {f['n_sources']} {f['n_targets']} {f['n_proposals']} {f['n_fused']} " + " ".join(_crc(a) for a in f["pairs"])


@pytest.mark.gpu
def test_cpp_program_equals_the_python_handle(gpu, tmp_path):
    from test_gpu_backend import _pack_cdr
    from dvslam_amd import PoseGraph
    from dvslam_amd.backend import MappingBackend
    scene = lc.scene()[0]
    (q, e, rvec, tvec, w_rot, w_trans), = lc.scene_loop()
    entries = [kf["frame_id"] for kf in scene[:3]]
    kpath, lpath = os.path.join(str(tmp_path), "keyframes.bin"), os.path.join(str(tmp_path), "loop.bin")
    with open(kpath, "wb") as fh:
        fh.write(struct.pack("<I", len(scene)))
        for kf in scene:
            payload = _pack_cdr(kf)
            fh.write(struct.pack("<I", len(payload)) + payload + struct.pack("<I", 0))
    with open(lpath, "wb") as fh:
        fh.write(struct.pack("<2Q10dI", q, e, *rvec, *tvec, w_rot, w_trans, *lc.ODO_W, len(entries)) + struct.pack(f"<{len(entries)}Q", *entries))
    out = subprocess.run([_build(tmp_path), kpath, lpath, repr(lc.FX), repr(lc.FY), repr(lc.CX), repr(lc.CY)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    mb = MappingBackend(lc.FX, lc.FY, lc.CX, lc.CY, filtered=("person",), initial_capacity=64)
    for kf in scene:
        mb.add_keyframe_cdr(_pack_cdr(kf), [])
    want = []
    ids, anc = mb.anchors()
    want.append(f"anchors {len(ids)} {_crc(ids)} {_crc(anc)}")
    g = mb.build_pose_graph(lc.scene_loop(), lc.ODO_W)
    want.append(f"graph {len(g['fixed'])} {len(g['ei'])} " + " ".join(_crc(g[k]) for k in ("R", "t", "fixed", "ei", "ej", "rvec", "tvec", "w_rot", "w_trans")))
    pg = PoseGraph()
    r = mb.close_loop(pg, lc.scene_loop(), lc.ODO_W)
    s = r["summary"]
    want.append(f"close term={s.termination} steps={s.num_successful_steps} its={s.num_iterations} pcg={s.pcg_iterations} "
                f"cost={struct.pack('>d', s.initial_cost).hex()},{struct.pack('>d', s.final_cost).hex()} nodes={r['n_nodes']} edges={r['n_edges']} "
                f"moved={r['n_landmarks_moved']} fused={r['n_fused']} " + _map_text(mb))
    dry = mb.fuse(q, entries, apply=False)
    want.append(_fuse_text("dry", dry) + " " + _map_text(mb))
    app = mb.fuse(q, entries, apply=True)
    want.append(_fuse_text("fuse", app) + " " + _map_text(mb))
    pg.close(); mb.close()
    got = out.stdout.strip().splitlines()
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a == b
    assert s.termination == 0 and app["n_fused"] >= 100 and dry["pairs"][1].tolist() == app["pairs"][1].tolist()
