"""C++ adapters: SlidingWindowBA::setDeviceWindow (include/dvslam/sliding_window_ba.hpp and the reference-named class of
include/dynamic_visual_slam/bundle_adjustment.hpp).  CPU: both compile with g++ -Wall -Werror against the C-ABI; GPU: the 20-keyframe
window runs on the device solver once the window is raised, silently, and gives the host path's cost."""
import os
import re
import subprocess
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "dynamic-visual-slam_amd", "lib")


def _build(tmpdir, opencv=False):
    exe = os.path.join(str(tmpdir), "ba_window_adapter" + ("_cv" if opencv else ""))
    extra = ["-DDVSLAM_WITH_OPENCV", "-I" + os.path.join(ROOT, "tests", "cpp", "stubs")] if opencv else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include")] + extra +
                          [os.path.join(ROOT, "tests", "cpp", "ba_window_adapter.cpp"), "-o", exe, "-L" + LIBDIR, "-ldvslam_hip",
                           "-Wl,-rpath," + LIBDIR, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


@pytest.mark.parametrize("opencv", [False, True], ids=["plain", "reference-named class"])
def test_adapter_compiles_and_refuses_without_gpu(tmp_path, hiplib, opencv):
    from dvslam_amd import device_count
    assert subprocess.call([_build(tmp_path, opencv), "window"], stdout=subprocess.DEVNULL) == (0 if device_count() > 0 else 3)


@pytest.mark.gpu
def test_raised_window_runs_on_the_device_solver(tmp_path, gpu, hiplib):
    exe = _build(tmp_path)
    host = subprocess.run([exe, "default"], capture_output=True, text=True)
    dev = subprocess.run([exe, "window"], capture_output=True, text=True)
    assert host.returncode == 0 and dev.returncode == 0, host.stdout + host.stderr + dev.stdout + dev.stderr
    assert "solving the normal equations on the host" in host.stderr and "1..16 of them free" in host.stderr
    assert dev.stderr == ""
    get = lambda out: (int(re.search(r"solver=(\d)", out).group(1)), float(re.search(r"cost=(\S+)", out).group(1)))   # noqa: E731
    (sh, ch), (sd, cd) = get(host.stdout), get(dev.stdout)
    assert (sh, sd) == (2, 1)
    assert abs(cd - ch) <= 1e-9 * ch, (cd, ch)
