"""C++ adapter dvslam::PoseGraph (include/dvslam/pose_graph.hpp: addNode, addEdge, addLoop, optimize, pose, correctPoints):
tests/cpp/pose_graph_adapter.cpp compiles with g++ -std=c++17 -Wall -Werror against the C-ABI (tests/test_pose_graph_cpu.py checks that
and the refusal without a GPU) and on the GPU prints the same bytes the Python binding returns for the same graph and points.  The adapter
hands a rotation matrix to the C-ABI as its principal rotation vector (the rule's Log); the binding is given that vector, made here from
the same matrix by the same operations through the C library's sqrt and atan2 (Python's math module), which is what the adapter calls —
numpy's arctan2 may differ from it in the last bit."""
import math
import struct
import subprocess
import numpy as np
import pytest

import pose_graph_ref as pr
from test_pose_graph_cpu import _build_adapter


def _rotation_vector(R):
    """dvslam::PoseGraph::rotationVector, operation by operation"""
    v = [(R[2, 1] - R[1, 2]) / 2, (R[0, 2] - R[2, 0]) / 2, (R[1, 0] - R[0, 1]) / 2]
    s = math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); c = (R[0, 0] + R[1, 1] + R[2, 2] - 1) / 2
    k = math.atan2(s, c) / s if s > 1e-12 else 1.0
    return [float(x) * k for x in v]


@pytest.mark.gpu
def test_cpp_adapter_program_equals_the_python_binding(gpu, tmp_path):
    from dvslam_amd import PoseGraph
    g = pr.graph("ring24")
    Rz = np.array([pr.rodrigues(w) for w in g.rvec])
    gpath, ppath = tmp_path / "graph.bin", tmp_path / "points.bin"
    gpath.write_bytes(struct.pack("<iii", g.N, g.E, 3) + g.R.tobytes() + g.t.tobytes() + g.fixed.tobytes() + g.ei.tobytes() + g.ej.tobytes() +
                      Rz.tobytes() + g.tvec.tobytes() + g.w_rot.tobytes() + g.w_trans.tobytes())
    rng = np.random.default_rng(21)
    xyz = rng.uniform(-6, 6, (50, 3)).astype(np.float32)
    anchor = rng.integers(-1, g.N + 1, 50).astype(np.int32)
    ppath.write_bytes(struct.pack("<i", len(xyz)) + xyz.tobytes() + anchor.tobytes())
    out = subprocess.run([_build_adapter(tmp_path), str(gpath), str(ppath)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr + out.stdout
    lines = [ln.split() for ln in out.stdout.strip().splitlines()]

    pg = PoseGraph()
    rvec = np.array([_rotation_vector(R) for R in Rz])
    pg.set_nodes(g.R, g.t, g.fixed).set_edges(g.ei, g.ej, rvec, g.tvec, g.w_rot, g.w_trans)
    cost0 = pg.evaluate()[0]
    s = pg.solve(**pr.TIGHT)
    R, t = pg.nodes()
    pts = pg.correct_points(xyz, anchor)
    ntrace = len(pg.trace())
    pg.close()
    hexd = lambda x: struct.pack(">d", float(x)).hex()
    hexf = lambda x: struct.pack(">f", float(x)).hex()
    assert lines[0] == ["cost", hexd(cost0)]
    assert lines[1] == ["summary"] + [str(v) for v in (s.termination, s.num_successful_steps, s.num_iterations, s.pcg_iterations)] + \
        [hexd(s.initial_cost), hexd(s.final_cost)]
    poses = [ln for ln in lines if ln[0] == "pose"]
    assert len(poses) == g.N
    for n, ln in enumerate(poses):
        assert ln[1] == str(n) and ln[2:] == [hexd(v) for v in R[n].ravel()] + [hexd(v) for v in t[n]]
    assert ["trace", str(ntrace)] in lines and lines[-1] == ["unverified", "refused"]
    points = [ln for ln in lines if ln[0] == "point"]
    assert len(points) == len(xyz)
    for k, ln in enumerate(points):
        assert ln[2:] == [hexf(v) for v in pts[k]]
    assert abs(s.final_cost - pr.SCIPY_COST["ring24"]) <= 1e-6 * s.final_cost and (pts != xyz).any()
