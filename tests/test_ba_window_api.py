"""CPU: the device-window option of the bundle adjustment (dvs_ba_set_device_window) is declared, exported, argument-checked without a
GPU, and the Python mirror refuses values outside 1..63 before any GPU call."""
import os
import re
import subprocess
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_declared_and_exported(hiplib, hooks):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dvslam_hip.h")).read(), flags=re.S)
    for name in ("dvs_ba_set_device_window", "dvs_ba_get_device_window"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(hiplib, name) and hasattr(hooks, name), name
    # the factorisation probe is a hook of the test library only
    thdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dvslam_hip_test.h")).read(), flags=re.S)
    assert re.search(r"\bdvs_ba_factor_probe\s*\(", thdr) and not re.search(r"\bdvs_ba_factor_probe\b", hdr)
    assert hasattr(hooks, "dvs_ba_factor_probe") and not hasattr(hiplib, "dvs_ba_factor_probe")
    exported = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "dynamic-visual-slam_amd", "lib", "libdvslam_hip.so")],
                              capture_output=True, text=True, check=True).stdout
    assert " T dvs_ba_set_device_window" in exported and "dvs_ba_factor_probe" not in exported


def test_null_handle_is_an_argument_error(hiplib):
    assert hiplib.dvs_ba_set_device_window(None, 32) == -6            # DVS_ERR_ARG, no device needed
    assert hiplib.dvs_ba_get_device_window(None) == 0


@pytest.mark.parametrize("bad", [0, 64, -3, 1000])
def test_python_mirror_refuses_out_of_range_before_any_gpu_call(bad):
    from dvslam_amd import SlidingWindowBA
    with pytest.raises(ValueError):
        SlidingWindowBA(900, 900, 640, 360, device_window=bad)


def test_python_mirror_default_and_range():
    from dvslam_amd import SlidingWindowBA
    assert SlidingWindowBA(900, 900, 640, 360).device_window == 16
    assert SlidingWindowBA(900, 900, 640, 360, device_window=63).device_window == 63
    assert SlidingWindowBA(900, 900, 640, 360, device_window=1).device_window == 1
