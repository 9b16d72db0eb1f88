"""Device time of dvs_triangulate_landmarks_device (csrc/triangulate.hip) on three workloads: 2 000 landmarks x 8 views, 100 000 landmarks
of 1..14 views (the GPU test's mix), and one landmark with 300 views.  Scenes come from tests/triangulate_ref.py (seeded), inputs stay
resident in HBM.  Prints one JSON line per workload: the median of `--iters` calls, each timed with the host clock around the call and
the synchronise that ends it (the call reads view_offsets[nlm] back before the launch, so the time includes that 8-byte copy and a
launch).  Every workload's result is checked bit for bit against the restatement once.
For kernel times alone run it under `rocprofv3 --kernel-trace --stats -d DIR -- python tools/time_triangulate.py`."""
import argparse
import json
import os
import sys
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dynamic-visual-slam_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import triangulate_ref as tr  # noqa: E402
from dvslam_amd import device_count  # noqa: E402
from dvslam_amd._lib import DeviceBuffer, check, lib  # noqa: E402
from dvslam_amd.glue import FrontendGlue  # noqa: E402


def workloads():
    rng = np.random.default_rng(7)
    R, t, _ = tr.keyframes(rng, 64, span=3.0)
    yield "2000 landmarks x 8 views", R, t, tr.random_landmarks(rng, R, t, 2000, 8, 8, noise=0.7)[:4]
    yield "100000 landmarks x 1..14 views", R, t, tr.random_landmarks(rng, R, t, 100_000, 1, 14, noise=1.5, perturb=0.2, skip=0.05, depth=(1.0, 12.0))[:4]
    yield "1 landmark x 300 views", R, t, tr.random_landmarks(rng, R, t, 1, 300, 300, noise=0.7)[:4]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    assert device_count() >= 1, "needs the MI355X"
    g = FrontendGlue(); L = lib(); h = g._h
    for name, R, t, (offs, vkf, vpx, xyz) in workloads():
        bufs = [DeviceBuffer(max(x.nbytes, 4)).upload(x) for x in (R, t, offs, vkf, vpx, xyz)]
        d_out = DeviceBuffer(xyz.nbytes); d_st = DeviceBuffer(len(xyz) * 4)
        dR, dt, do, dk, dp, dx = (b.ptr for b in bufs)
        args = (h, len(R), dR, dt, *tr.K4, len(xyz), do, dk, dp, dx, d_out.ptr, d_st.ptr)
        for _ in range(a.warmup):
            check(L.dvs_triangulate_landmarks_device(*args))
        check(L.dvs_matcher_synchronize(h))
        ms = []
        for _ in range(a.iters):
            t0 = time.perf_counter()
            check(L.dvs_triangulate_landmarks_device(*args))
            check(L.dvs_matcher_synchronize(h))
            ms.append((time.perf_counter() - t0) * 1e3)
        want, wst = tr.triangulate(R, t, *tr.K4, offs, vkf, vpx, xyz)
        got = d_out.download(np.float32, xyz.size).reshape(-1, 3); st = d_st.download(np.int32, len(xyz))
        assert got.tobytes() == want.tobytes() and (st == wst).all(), name
        print(json.dumps(dict(workload=name, landmarks=len(xyz), views=int(offs[-1]), call_ms_median=round(float(np.median(ms)), 4),
                              call_ms_min=round(float(np.min(ms)), 4), iters=a.iters, updated=int((st == 0).sum()))), flush=True)


if __name__ == "__main__":
    main()
