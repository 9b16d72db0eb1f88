"""include/dvslam/triangulation.hpp: associateAndTriangulate (one batched dvs_triangulate_landmarks, then the sequential walk) against the
reference's one-by-one loop, which triangulates each matched landmark at match time (tests/cpp/triangulate_assoc.cpp)."""
import subprocess
import pytest
from test_adapters_and_dist import _build_cpp


def test_triangulation_adapter_compiles(tmp_path, hiplib):
    from dvslam_amd import device_count
    assert subprocess.call([_build_cpp(tmp_path, "triangulate_assoc.cpp", "triangulate_assoc")]) == (0 if device_count() > 0 else 3)


@pytest.mark.gpu
def test_associate_and_triangulate_matches_the_one_by_one_loop(tmp_path, gpu, hiplib):
    out = subprocess.run([_build_cpp(tmp_path, "triangulate_assoc.cpp", "triangulate_assoc")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "adapter vs one-by-one loop: 0 differences, db equal 1" in out.stdout and "obs1 -> 210 (snapshot 5)" in out.stdout
