"""Times the covisibility calls of the mapping backend (csrc/covisibility.hip) on one GPU.
    python tools/covisibility_timing.py [--reps 20] [--out FILE.json]
Maps, the shapes of tools/global_ba_timing.py built through dvs_backend_add_keyframe (exact projections, every world point its own random
descriptor, so the association follows the geometry):
  full     64 keyframes x 2000 landmarks, every keyframe sees every landmark
  banded   1024 keyframes x 3072 landmarks along a corridor, the camera stepping 0.2 m: a landmark is seen by about 25 keyframes
Every figure is WALL time of a blocking call in ms, the median (min .. max) of `reps` calls after two warm-up calls:
  graph          MappingBackend.covisibility(15): all rows, the neighbour lists and the read-back of the n x n weights
  graph_lists    the same without the weights' read-back
  one_row        MappingBackend.local_window(newest, max_neighbours=0, max_fixed=0): the CSRs, ONE row of weights, its neighbour list, U
  local_window   MappingBackend.local_window(newest) with the defaults, read-back of the window included
  track_local    MappingBackend.track_frame_local(newest) on the newest keyframe's own observations as keypoints
  track_whole    MappingBackend.track_frame on the same frame: the whole-table path, which the covisibility calls did not change
No time is promised for any of them; EXPERIMENTS.md "Covisibility" says what has been run."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dynamic-visual-slam_amd"))
FX = FY = 500.0; CX, CY = 320.0, 240.0
Q_Z180 = (0.0, 0.0, 1.0, 0.0)


def stats(ms):
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def timed(reps, call):
    ms = []
    for rep in range(reps + 2):
        t0 = time.perf_counter(); call(); t1 = time.perf_counter()
        if rep >= 2:
            ms.append((t1 - t0) * 1e3)
    return stats(ms)


def keyframes(shape, seed=5):
    rng = np.random.default_rng(seed)
    if shape == "full":
        nkf, npts, step = 64, 2000, 0.01
        X = np.stack([rng.uniform(-0.8, 1.4, npts), rng.uniform(-0.8, 0.8, npts), rng.uniform(3.2, 5.0, npts)], 1)
    else:
        nkf, npts, step = 1024, 3072, 0.2
        X = np.stack([rng.uniform(-2.0, step * nkf + 2.0, npts), rng.uniform(-0.8, 0.8, npts), rng.uniform(3.2, 5.0, npts)], 1)
    D = rng.integers(0, 256, (npts, 32), dtype=np.uint8)
    for k in range(nkf):
        t = np.array([step * k, 0.0, 0.0])
        xc = np.stack([-X[:, 0] + t[0], -X[:, 1] + t[1], X[:, 2]], 1)
        u = FX * xc[:, 0] / xc[:, 2] + CX; v = FY * xc[:, 1] / xc[:, 2] + CY
        vis = np.nonzero((u > 8) & (u < 632) & (v > 8) & (v < 472))[0]
        yield dict(frame_id=100 + k, stamp=(10 + k, 0), t=t, q=Q_Z180, xyz=X[vis], px=np.stack([u[vis], v[vis]], 1), desc=D[vis])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from dvslam_amd import map_track as M
    from dvslam_amd._lib import DeviceBuffer, KP_DTYPE
    from dvslam_amd.backend import MappingBackend
    res = {"clock": "wall, blocking calls", "reps": a.reps, "maps": []}
    for shape in ("full", "banded"):
        mb = MappingBackend(FX, FY, CX, CY, filtered=())
        last = None
        for kf in keyframes(shape):
            mb.add_keyframe(kf["frame_id"], kf["stamp"], kf["t"], kf["q"], kf["xyz"], kf["px"], kf["desc"])
            last = kf
        c = mb.counts()
        g = mb.covisibility(15)
        newest = last["frame_id"]
        w = mb.local_window(newest)
        row = {"shape": shape, "keyframes": c["n_keyframes"], "landmarks": c["n_landmarks"], "observations": c["n_observations"],
               "neighbours_at_15": int(len(g["nb_index"])), "window": {"keyframes": int(len(w["kf_frame_id"])), "fixed": int(w["kf_fixed"].sum()),
                                                                      "landmarks": int(len(w["lm_id"])), "observations": int(len(w["obs_px"]))}}
        row["graph"] = timed(a.reps, lambda: mb.covisibility(15))
        row["graph_lists"] = timed(a.reps, lambda: mb.covisibility(15, weights=False))
        row["one_row"] = timed(a.reps, lambda: mb.local_window(newest, max_neighbours=0, max_fixed=0))
        row["local_window"] = timed(a.reps, lambda: mb.local_window(newest))
        n = len(last["px"])
        kps = np.zeros(n, KP_DTYPE); kps["x"] = last["px"][:, 0]; kps["y"] = last["px"][:, 1]; kps["size"] = 31.0
        mt = M.MapTracker(M.default_params(480, 640, FX, FY, CX, CY))
        d_k, d_d = DeviceBuffer(kps.nbytes).upload(kps), DeviceBuffer(last["desc"].nbytes).upload(last["desc"])
        R = np.diag([-1.0, -1.0, 1.0]); t = np.asarray(last["t"], np.float64) + np.array([0.01, -0.008, 0.012])
        local = mb.track_frame_local(mt, newest, d_k, d_d, n, R, t)
        whole = mb.track_frame(mt, d_k, d_d, n, R, t)
        row["track"] = {"keypoints": n, "local": {k: local[k] for k in ("status", "n_visible", "n_matches", "n_inliers")},
                        "whole": {k: whole[k] for k in ("status", "n_visible", "n_matches", "n_inliers")}}
        row["track_local"] = timed(a.reps, lambda: mb.track_frame_local(mt, newest, d_k, d_d, n, R, t))
        row["track_whole"] = timed(a.reps, lambda: mb.track_frame(mt, d_k, d_d, n, R, t))
        d_k.free(); d_d.free(); mt.close(); mb.close()
        res["maps"].append(row)
        print(json.dumps(row), flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
