"""C++ adapter include/dvslam/landmark_culling.hpp: tests/cpp/landmark_culling.cpp compiles with g++ -std=c++17 -Wall -Werror against the
C-ABI and refuses to run without a GPU (exit code 3); on the GPU, fed the moved-object scene of tests/landmark_culling_ref.py from files, it
writes the same text — the statistics before and after the recording, a dry-run cull, the applied cull and the CRC-32 of every table
column after it — as the Python handle."""
import os
import struct
import subprocess
import zlib
import numpy as np
import pytest

import backend_ref as br
import landmark_culling_ref as lcr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "dynamic-visual-slam_amd", "lib")


def _build(tmpdir):
    exe = os.path.join(str(tmpdir), "landmark_culling")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "landmark_culling.cpp"),
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


def _stats_text(tag, mb):
    s = mb.landmark_stats()
    return f"{tag} {len(s['id'])} {s['n_frames_recorded']} " + " ".join(_crc(s[k]) for k in ("id", "visible", "found", "n_views", "age_kf"))


def _report_text(tag, r):
    return (f"{tag} {r['n_landmarks']} {r['n_by_ratio']} {r['n_weak']} {r['n_landmarks_removed']} {r['n_observations_removed']} {r['n_keyframes_touched']} "
            f"{len(r['culled_id'])} {_crc(r['culled_id'])} {_crc(r['culled_reason'])}")


@pytest.mark.gpu
def test_cpp_program_equals_the_python_handle(gpu, tmp_path):
    from test_gpu_backend import _pack_cdr
    from dvslam_amd import map_track as M
    from dvslam_amd._lib import DeviceBuffer
    from dvslam_amd.backend import MappingBackend
    kfs, q = lcr.object_scene()
    n_frames = lcr.DEFAULTS["min_visible"]
    kpath, fpath = os.path.join(str(tmp_path), "keyframes.bin"), os.path.join(str(tmp_path), "frame.bin")
    with open(kpath, "wb") as fh:
        fh.write(struct.pack("<I", len(kfs)))
        for kf in kfs:
            payload = _pack_cdr(kf)
            fh.write(struct.pack("<I", len(payload)) + payload + struct.pack("<I", 0))
    with open(fpath, "wb") as fh:
        fh.write(struct.pack("<I", len(q["kps"])) + q["kps"].tobytes() + np.ascontiguousarray(q["kdesc"]).tobytes() +
                 np.ascontiguousarray(q["R"], np.float64).tobytes() + np.ascontiguousarray(q["t"], np.float64).tobytes())
    out = subprocess.run([_build(tmp_path), kpath, fpath, repr(br.FX), repr(br.FY), repr(br.CX), repr(br.CY), str(n_frames)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    mb = MappingBackend(br.FX, br.FY, br.CX, br.CY, filtered=("person",), initial_capacity=64)
    for kf in kfs:
        mb.add_keyframe_cdr(_pack_cdr(kf), [])
    mt = M.MapTracker(M.default_params(480, 640, br.FX, br.FY, br.CX, br.CY))
    d_k, d_d = DeviceBuffer(q["kps"].nbytes).upload(q["kps"]), DeviceBuffer(q["kdesc"].nbytes).upload(q["kdesc"])
    want = [_stats_text("before", mb)]
    mb.set_tracking_stats(True)
    for _ in range(n_frames):
        r = mb.track_frame(mt, d_k, d_d, len(q["kps"]), q["R"], q["t"])
        want.append(f"track {r['status']} {r['n_visible']} {r['n_matches']} {r['n_inliers']}")
    want.append(_stats_text("recorded", mb))
    dry = mb.cull_landmarks(apply=False)
    want.append(_report_text("dry", dry)); want.append(_map_text(mb))
    rep = mb.cull_landmarks()
    assert rep["n_landmarks_removed"] == lcr.OBJECT_N == dry["n_by_ratio"] and dry["n_landmarks_removed"] == 0
    want.append(_report_text("cull", rep)); want.append(_stats_text("after", mb)); want.append(_map_text(mb))
    s = mb.landmark_stats()
    mb.clear_landmark_stats()
    want.append(_stats_text("cleared", mb))
    mb.set_landmark_stats(s["id"], s["visible"], s["found"])
    want.append(_stats_text("restored", mb))
    assert want[-1].split()[3:] == want[-4].split()[3:] and want[-2] != want[-1]
    assert out.stdout.splitlines() == want
    d_k.free(); d_d.free(); mt.close(); mb.close()
