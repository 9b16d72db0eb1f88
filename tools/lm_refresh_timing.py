"""Times the landmark refresh on the mapping backend (csrc/landmark_refresh.hip, the gates in csrc/map_track.hip) on one GPU.
    python tools/lm_refresh_timing.py [--reps 20] [--out FILE.json]                 wall times
    python tools/lm_refresh_timing.py --mode profile --dir DIR [--out FILE.json]    per-kernel times of dry refreshes: starts
                                                                                    `rocprofv3 --kernel-trace --stats` on --mode kernels
Maps, those of tools/covisibility_timing.py (built through dvs_backend_add_keyframe, exact projections, every world point its own random
descriptor):
  full     64 keyframes x 2000 landmarks, every keyframe sees every landmark: every landmark has 64 views, all on the wavefront path
  banded   1024 keyframes x 3072 landmarks along a corridor: a landmark is seen by about 25 keyframes
  hub      the hub scene of the tests: 300 keyframes, one landmark seen by all of them — the one workgroup of the third path
Wall figures are ms of a blocking call, the median (min .. max) of `reps` calls after two warm-up calls:
  refresh_dry    MappingBackend.refresh_landmarks(update_descriptors=0): the views, the bins, the three selections, the comparison
  refresh        the same with the write (on these maps every view of a point carries one descriptor, so nothing changes)
  refresh_scope  the newest keyframe's landmarks only
  geometry       MappingBackend.landmark_geometry(): views, selection, geometry, and five columns copied to the host
  track_gated    MappingBackend.track_frame_gated on the newest keyframe's own keypoints with a prior 1-2 cm off
  track_whole    MappingBackend.track_frame on the same input, the same run: what the gates' per-call geometry costs on top
No time is promised for any of them; EXPERIMENTS.md "Landmark refresh" says what has been run."""
import argparse
import glob
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dynamic-visual-slam_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from covisibility_timing import FX, FY, CX, CY, keyframes, timed    # noqa: E402

PROFILE_RUNS = 20


def build(shape):
    from dvslam_amd.backend import MappingBackend
    mb = MappingBackend(FX, FY, CX, CY, filtered=())
    last = None
    if shape == "hub":
        import covisibility_ref as cr
        kfs = cr.hub_scene()
    else:
        kfs = keyframes(shape)
    for kf in kfs:
        mb.add_keyframe(kf["frame_id"], kf["stamp"], kf["t"], kf["q"], kf["xyz"], kf["px"], kf["desc"])
        last = kf
    return mb, last


def mode_wall(reps):
    from dvslam_amd import map_track as M
    from dvslam_amd._lib import DeviceBuffer, KP_DTYPE
    res = {"clock": "wall, blocking calls", "reps": reps, "maps": []}
    for shape in ("full", "banded", "hub"):
        mb, last = build(shape)
        c = mb.counts()
        newest = last["frame_id"]
        rep = mb.refresh_landmarks(update_descriptors=0)
        row = {"shape": shape, "keyframes": c["n_keyframes"], "landmarks": c["n_landmarks"], "observations": c["n_observations"], "report": rep,
               "scope_report": mb.refresh_landmarks(newest, update_descriptors=0)}
        row["refresh_dry"] = timed(reps, lambda: mb.refresh_landmarks(update_descriptors=0))
        row["refresh"] = timed(reps, lambda: mb.refresh_landmarks())
        row["refresh_scope"] = timed(reps, lambda: mb.refresh_landmarks(newest))
        row["geometry"] = timed(reps, lambda: mb.landmark_geometry())
        n = len(last["px"])
        kps = np.zeros(n, KP_DTYPE); kps["x"] = last["px"][:, 0]; kps["y"] = last["px"][:, 1]; kps["size"] = 31.0
        mt = M.MapTracker(M.default_params(480, 640, FX, FY, CX, CY))
        d_k, d_d = DeviceBuffer(kps.nbytes).upload(kps), DeviceBuffer(last["desc"].nbytes).upload(last["desc"])
        R = np.diag([-1.0, -1.0, 1.0]); t = np.asarray(last["t"], np.float64) + np.array([0.01, -0.008, 0.012])
        gated = mb.track_frame_gated(mt, d_k, d_d, n, R, t)
        counts = mt.gate_counts().tolist()
        whole = mb.track_frame(mt, d_k, d_d, n, R, t)
        row["track"] = {"keypoints": n, "gate_counts": counts, "gated": {k: gated[k] for k in ("status", "n_visible", "n_matches", "n_inliers")},
                        "whole": {k: whole[k] for k in ("status", "n_visible", "n_matches", "n_inliers")}}
        row["track_gated"] = timed(reps, lambda: mb.track_frame_gated(mt, d_k, d_d, n, R, t))
        row["track_whole"] = timed(reps, lambda: mb.track_frame(mt, d_k, d_d, n, R, t))
        d_k.free(); d_d.free(); mt.close(); mb.close()
        res["maps"].append(row)
        print(json.dumps(row), flush=True)
    return res


def mode_kernels(shape):
    """what the profile traces: PROFILE_RUNS dry refreshes and as many geometry reads, after the map is built"""
    mb, _ = build(shape)
    for _ in range(PROFILE_RUNS):
        rep = mb.refresh_landmarks(update_descriptors=0)
        mb.landmark_geometry()
    mb.close()
    return {"runs": PROFILE_RUNS, "report": rep}


def mode_profile(out_dir, shape):
    import csv
    os.makedirs(out_dir, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out_dir, "-o", "lm_refresh", "--", sys.executable, os.path.abspath(__file__),
           "--mode", "kernels", "--shape", shape]
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=560)
    if run.returncode != 0:
        raise SystemExit(f"rocprofv3 failed ({run.returncode}):\n{run.stdout[-2000:]}\n{run.stderr[-2000:]}")
    files = glob.glob(os.path.join(out_dir, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no kernel statistics under {out_dir}")
    rows = []
    for r in csv.DictReader(open(files[0])):
        name = r.get("Name", "").split("(")[0]
        if "k_lr_" in name:                             # the views CSR's kernels also serve the map's construction and cannot be told apart by name
            rows.append({"kernel": name, "calls": int(r["Calls"]), "average_us": round(float(r["AverageNs"]) / 1e3, 2), "min_us": round(float(r["MinNs"]) / 1e3, 2),
                         "max_us": round(float(r["MaxNs"]) / 1e3, 2)})
    return {"shape": shape, "runs": PROFILE_RUNS, "source": os.path.relpath(files[0], out_dir), "kernels": rows,
            "note": "the kernels of landmark_refresh.hip over 20 dry refreshes and 20 geometry reads (a read selects as well: 40 calls of the selection kernels); on the hub "
                    "map k_lr_select_block's one busy workgroup is the landmark of 300 views on its own"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("wall", "kernels", "profile"), default="wall")
    ap.add_argument("--shape", choices=("full", "banded", "hub"), default="hub")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--dir", default="lm_refresh_profile")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = mode_wall(a.reps) if a.mode == "wall" else mode_kernels(a.shape) if a.mode == "kernels" else mode_profile(a.dir, a.shape)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
