"""C++ adapter dvslam::TrackingFrontend (include/dvslam/tracking_frontend.hpp): tests/cpp/tracker_adapter.cpp compiles with
g++ -std=c++17 -Wall -Werror against the C-ABI, plain and with the cv::Mat overload over the OpenCV stubs, and refuses to run without a
GPU (exit code 3) as the other adapter programs do.  The GPU run is tests/test_gpu_tracker.py's."""
import os
import subprocess
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "dynamic-visual-slam_amd", "lib")


def _build(tmpdir, opencv):
    exe = os.path.join(str(tmpdir), "tracker_adapter" + ("_cv" if opencv else ""))
    extra = ["-DDVSLAM_WITH_OPENCV", "-I" + os.path.join(ROOT, "tests", "cpp", "stubs")] if opencv else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include")] + extra +
                          [os.path.join(ROOT, "tests", "cpp", "tracker_adapter.cpp"), "-o", exe, "-L" + LIBDIR, "-ldvslam_hip",
                           "-Wl,-rpath," + LIBDIR, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


@pytest.mark.parametrize("opencv", [False, True], ids=["plain", "cv::Mat overload"])
def test_adapter_compiles_and_refuses_without_gpu(tmp_path, hiplib, opencv):
    from dvslam_amd import device_count
    code = subprocess.call([_build(tmp_path, opencv)], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    assert code == (2 if device_count() > 0 else 3)       # with a GPU and no arguments: the usage exit
