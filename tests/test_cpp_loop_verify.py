"""C++ adapter dvslam::LoopDatabase, verification layer (include/dvslam/loop_detection.hpp: setPoints, getPoints, verify,
detectVerified): tests/cpp/loop_verify_adapter.cpp compiles with g++ -std=c++17 -Wall -Werror against the C-ABI, refuses to run without a
GPU (exit code 3), and on the GPU prints per candidate what the Python binding returns for the same frames and points: integers, the
bytes of t and rms, the inlier rows; R (which the adapter makes from the Rodrigues vector on the host) to 1e-12."""
import os
import struct
import subprocess
import numpy as np
import pytest

import bow_ref as br
import loop_ref as lr
import loop_verify_ref as vr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "dynamic-visual-slam_amd", "lib")


def _build(tmpdir):
    exe = os.path.join(str(tmpdir), "loop_verify_adapter")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "loop_verify_adapter.cpp"), "-o", exe, "-L" + LIBDIR, "-ldvslam_hip",
                           "-Wl,-rpath," + LIBDIR, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_adapter_compiles_and_refuses_without_gpu(tmp_path, hiplib):
    from dvslam_amd import device_count
    code = subprocess.call([_build(tmp_path)], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    assert code == (2 if device_count() > 0 else 3)       # with a GPU and no arguments: the usage exit


def _hex(x):
    return struct.pack(">d", float(x)).hex()


def _parse(lines):
    """{tag: [candidate dict]} of the adapter's output"""
    out, cur = {}, None
    for ln in lines:
        w = ln.split()
        if w[0] != "cand":
            cur = out.setdefault(w[0], []); assert int(w[1]) >= 0
            continue
        r0 = w.index("R")
        k = w.index("inliers")
        cur.append(dict(id=int(w[1]), verified=int(w[2]), n_corr=int(w[3]), iterations=int(w[4]), n_matches=int(w[5]), t=w[7:10], rms=w[11],
                        R=np.array([float(x) for x in w[r0 + 1:r0 + 10]]).reshape(3, 3), inliers=[int(x) for x in w[k + 2:]], n_in=int(w[k + 1])))
    return out


@pytest.mark.gpu
def test_cpp_adapter_program_equals_the_python_binding(gpu, tmp_path):
    from dvslam_amd import OrbVocabulary, LoopDatabase, LoopVerifyParams
    voc, entries, query = lr.standard_scene()
    ref = lr.LoopDatabase(voc, 1)
    for e in entries:
        ref.add(e)
    train = ref.match(query, [0, 1, 2, 3])[0]
    pts, qp = vr.standard_points(entries, query, train[1])
    vpath, fpath, ppath = tmp_path / "ORBvoc.txt", tmp_path / "frames.bin", tmp_path / "points.bin"
    br.write_text(voc, vpath)
    frames, clouds = entries + [query], pts + [qp]
    fpath.write_bytes(struct.pack("<i", len(frames)) + b"".join(struct.pack("<i", len(f)) + f.tobytes() for f in frames))
    ppath.write_bytes(struct.pack("<i", len(clouds)) + b"".join(struct.pack("<i", len(c)) + c.tobytes() for c in clouds))
    out = subprocess.run([_build(tmp_path), str(vpath), str(fpath), str(ppath), "3"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr + out.stdout
    got = _parse(out.stdout.strip().splitlines())
    g = OrbVocabulary.from_arrays(voc.k, voc.L, voc.parent, voc.is_leaf, voc.desc, voc.weight, voc.scoring, voc.weighting)
    db = LoopDatabase(g, 1)
    for k, e in enumerate(entries):
        db.add(e)
        if k != 2:
            db.set_points(k, pts[k])
    P = LoopVerifyParams(vr.K4, iterations=64, seed=3)
    ids, scores, nm, tr, dist, res, mask = db.detect_verify(query, qp, P, 3)
    mt, _, mn = db.match(query, [0, 1, 2, 3])
    res2, mask2 = db.verify(qp, [0, 1, 2, 3], mt, P)
    for tag, wids, wnm, wres, wmask in (("detectVerified", ids, nm, res, mask), ("verify", [0, 1, 2, 3], mn, res2, mask2)):
        assert [c["id"] for c in got[tag]] == [int(x) for x in wids]
        for c, n_m, r, m in zip(got[tag], wnm, wres, wmask):
            assert (c["verified"], c["n_corr"], c["iterations"], c["n_matches"]) == (int(r["success"]), int(r["n_corr"]), int(r["iterations"]), int(n_m))
            assert c["t"] == [_hex(x) for x in r["tvec"]] and c["rms"] == _hex(r["rms_px"])
            assert c["inliers"] == np.flatnonzero(m).tolist() and c["n_in"] == int(r["n_inliers"])
            a = np.linalg.norm(r["rvec"])
            want = np.eye(3) if a == 0 else vr._rot(r["rvec"], a)
            assert np.abs(c["R"] - want).max() <= 1e-12
    v = {c["id"]: c for c in got["verify"]}
    assert v[1]["verified"] == 1 and np.abs(v[1]["R"] - vr.POSE_R).max() < 1e-5 and v[2]["n_corr"] == 0 and v[2]["verified"] == 0
    db.close(); g.close()
