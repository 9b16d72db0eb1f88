"""C++ adapter dvslam::globalBundleAdjust (include/dvslam/global_ba.hpp): tests/cpp/global_ba_adapter.cpp compiles with g++ -std=c++17
-Wall -Werror against the C-ABI and refuses to run without a GPU (exit code 3); on the GPU, fed the arc map of
tests/test_gpu_backend_global_ba.py from a file, it writes the same text — the result of a capped and of a full run and the CRC-32 of the
columns they may touch — as the Python handle."""
import os
import struct
import subprocess
import zlib
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "dynamic-visual-slam_amd", "lib")


def _build(tmpdir):
    exe = os.path.join(str(tmpdir), "global_ba_adapter")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "global_ba_adapter.cpp"),
                           "-o", exe, "-L" + LIBDIR, "-ldvslam_hip", "-Wl,-rpath," + LIBDIR, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_adapter_compiles_and_refuses_without_gpu(tmp_path, hiplib):
    from dvslam_amd import device_count
    code = subprocess.call([_build(tmp_path)], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    assert code == (2 if device_count() > 0 else 3)       # with a GPU and no arguments: the usage exit


def _crc(a):
    return "%08x" % (zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xFFFFFFFF)


def _run_text(tag, r, mb):
    s = r["summary"]
    L, O, K = mb.landmarks(), mb.observations(), mb.keyframes()
    return (f"{tag} term={s.ba.termination} steps={s.ba.num_successful_steps} its={s.ba.num_iterations} solver={s.ba.linear_solver} pcg={s.pcg_iterations} "
            f"cost={struct.pack('>d', s.ba.initial_cost).hex()},{struct.pack('>d', s.ba.final_cost).hex()} cams={r['n_cameras']} lms={r['n_landmarks']} "
            f"obs={r['n_observations']} left={r['n_left_out']} lm={len(L['id'])} {_crc(L['id'])} {_crc(L['xyz'])} ob={len(O['id'])} {_crc(O['landmark_id'])} {_crc(O['px'])} "
            f"kf={len(K['frame_id'])} {_crc(K['R'])} {_crc(K['t'])}")


@pytest.mark.gpu
def test_cpp_program_equals_the_python_handle(gpu, tmp_path):
    from test_gpu_backend import _pack_cdr
    from test_gpu_backend_global_ba import arc_keyframes, FX, FY, CX, CY
    from dvslam_amd.backend import MappingBackend
    scene = arc_keyframes()
    kpath = os.path.join(str(tmp_path), "keyframes.bin")
    with open(kpath, "wb") as fh:
        fh.write(struct.pack("<I", len(scene)))
        for kf in scene:
            payload = _pack_cdr(kf)
            fh.write(struct.pack("<I", len(payload)) + payload + struct.pack("<I", 0))
    out = subprocess.run([_build(tmp_path), kpath, repr(FX), repr(FY), repr(CX), repr(CY)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    mb = MappingBackend(FX, FY, CX, CY, filtered=("person",), initial_capacity=64)
    for kf in scene:
        mb.add_keyframe_cdr(_pack_cdr(kf), [])
    want = [_run_text("capped", mb.global_bundle_adjust(max_iterations=1), mb)]
    r = mb.global_bundle_adjust()
    want.append(_run_text("global", r, mb))
    mb.close()
    got = out.stdout.strip().splitlines()
    assert got == want
    assert r["summary"].ba.termination == 0 and r["summary"].ba.linear_solver == 3
