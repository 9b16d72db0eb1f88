"""Times the landmark tracking statistics and the landmark cull on the mapping backend (csrc/lm_cull.hip, the recording in
csrc/map_track.hip) on one GPU.
    python tools/lm_cull_timing.py [--reps 20] [--out FILE.json]
Maps, those of tools/covisibility_timing.py (built through dvs_backend_add_keyframe, exact projections, every world point its own random
descriptor):
  full     64 keyframes x 2000 landmarks, every keyframe sees every landmark
  banded   1024 keyframes x 3072 landmarks along a corridor: a landmark is seen by about 25 keyframes
Wall figures are ms of a blocking call, the median (min .. max) of `reps` calls after two warm-up calls:
  track_off    MappingBackend.track_frame on the newest keyframe's own keypoints with a prior 1-2 cm off, the recording switched off: the
               call as it was before this section existed
  track_on     the same with the recording on: the alignment kernel, the record kernel and one more wait
  cull_dry     MappingBackend.cull_landmarks(apply=False): the alignment, the views, the decision, the ids copied to the host
  stats        MappingBackend.landmark_stats(): the alignment, the views and five columns copied to the host
  cull_apply   five applied culls in a row, each removing every tenth landmark of the map as it then stands (rule F through counters
               set for it): the compaction of both tables and the statistics and the host's cascade; each figure is one call
  prune        one MappingBackend.prune behind them that removes about a tenth of the landmarks (prune_line below), one call
No time is promised for any of them; EXPERIMENTS.md "Landmark culling" says what has been run."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dynamic-visual-slam_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from covisibility_timing import FX, FY, CX, CY, keyframes, timed    # noqa: E402


def build(shape):
    from dvslam_amd.backend import MappingBackend
    mb = MappingBackend(FX, FY, CX, CY, filtered=())
    last = None
    for kf in keyframes(shape):
        mb.add_keyframe(kf["frame_id"], kf["stamp"], kf["t"], kf["q"], kf["xyz"], kf["px"], kf["desc"])
        last = kf
    return mb, last


def prune_line(mb, last):
    """one dvs_backend_prune that removes about a tenth of the landmarks: a keyframe of points nobody has seen joins the map, a ninth as
    many as the map holds (one view each, behind every other row of both tables), and the prune comes 21 s after it"""
    n = max(mb.counts()["n_landmarks"] // 9, 1)
    rng = np.random.default_rng(77)
    px = np.stack([rng.uniform(20, 620, n), rng.uniform(20, 460, n)], 1)
    xyz = np.stack([rng.uniform(50, 60, n), rng.uniform(50, 60, n), rng.uniform(50, 60, n)], 1)      # far from every landmark of the map
    stamp = (last["stamp"][0] + 1000, 0)
    res = mb.add_keyframe(last["frame_id"] + 100000, stamp, last["t"], last["q"], xyz, px, rng.integers(0, 256, (n, 32), dtype=np.uint8))
    c = mb.counts()
    t0 = time.perf_counter()
    removed = mb.prune((stamp[0] + 21, 0))
    ms = (time.perf_counter() - t0) * 1e3
    return {"ms": round(ms, 3), "landmarks": c["n_landmarks"], "observations": c["n_observations"], "created": res["n_created"], "removed": list(removed)}


def mode_wall(reps):
    from dvslam_amd import map_track as M
    from dvslam_amd._lib import DeviceBuffer, KP_DTYPE
    res = {"clock": "wall, blocking calls", "reps": reps, "maps": []}
    keep = ("status", "n_visible", "n_matches", "n_inliers")
    for shape in ("full", "banded"):
        mb, last = build(shape)
        c = mb.counts()
        row = {"shape": shape, "keyframes": c["n_keyframes"], "landmarks": c["n_landmarks"], "observations": c["n_observations"]}
        n = len(last["px"])
        kps = np.zeros(n, KP_DTYPE); kps["x"] = last["px"][:, 0]; kps["y"] = last["px"][:, 1]; kps["size"] = 31.0
        mt = M.MapTracker(M.default_params(480, 640, FX, FY, CX, CY))
        d_k, d_d = DeviceBuffer(kps.nbytes).upload(kps), DeviceBuffer(last["desc"].nbytes).upload(last["desc"])
        R = np.diag([-1.0, -1.0, 1.0]); t = np.asarray(last["t"], np.float64) + np.array([0.01, -0.008, 0.012])
        off = mb.track_frame(mt, d_k, d_d, n, R, t)
        row["track"] = {"keypoints": n, "result": {k: off[k] for k in keep}}
        row["track_off"] = timed(reps, lambda: mb.track_frame(mt, d_k, d_d, n, R, t))
        mb.set_tracking_stats(True)
        row["track_on"] = timed(reps, lambda: mb.track_frame(mt, d_k, d_d, n, R, t))
        mb.set_tracking_stats(False)
        s = mb.landmark_stats()
        row["recorded"] = {"n_frames_recorded": s["n_frames_recorded"], "visible_rows": int((s["visible"] > 0).sum()), "found_rows": int((s["found"] > 0).sum())}
        dry = mb.cull_landmarks(apply=False)
        row["dry_report"] = {k: v for k, v in dry.items() if not isinstance(v, np.ndarray)}
        row["cull_dry"] = timed(reps, lambda: mb.cull_landmarks(apply=False))
        row["stats"] = timed(reps, lambda: mb.landmark_stats())
        applied = []
        for _ in range(5):
            ids = mb.landmarks()["id"]
            mb.clear_landmark_stats()
            mark = ids[::10]
            mb.set_landmark_stats(mark, np.full(len(mark), 8, np.int32), np.zeros(len(mark), np.int32))
            t0 = time.perf_counter()
            rep = mb.cull_landmarks(weak_age_kf=-1)
            ms = (time.perf_counter() - t0) * 1e3
            applied.append({"ms": round(ms, 3), "landmarks": len(ids), "removed": rep["n_landmarks_removed"], "observations_removed": rep["n_observations_removed"],
                            "keyframes_touched": rep["n_keyframes_touched"]})
        row["cull_apply"] = applied
        row["prune"] = prune_line(mb, last)
        d_k.free(); d_d.free(); mt.close(); mb.close()
        res["maps"].append(row)
        print(json.dumps(row), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    line = json.dumps(mode_wall(a.reps))
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
