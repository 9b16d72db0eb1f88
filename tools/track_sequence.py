#!/usr/bin/env python3
"""Drives the tracking front end (dvs_tracker_track: one call per RGB-D frame, device-resident) over the synthetic trajectory and prints
wall milliseconds per frame, beside the frame-by-frame loop over the one-stage host-pointer entry points (replay_tracking.track with
HipStages, pre=None) in the same process on the same frames.

What is compared.  The loop runs OpenCV's procedure in both fundamental-matrix gates (dvs_find_fundamental_cv) and the library's own PnP;
the tracker is therefore timed in that configuration (fm_mode = 1, pnp_mode = 0: the like-for-like figure) AND with its defaults
(fm_mode = 0: the library's own seeded estimator in the gates, which needs no read-back).  The loop's time is everything inside its frame
loop: the stage calls with their transfers and synchronisations, and also its Python — numpy glue, and the feature culling as a list
comprehension and a sort over every feature.  The tracker's time is the ctypes call, which includes copying the image and the depth image
into pinned memory.  The ratio says how the two ways of driving the stages compare for a caller; it does not split the difference into causes.
Warm-up frames run first through everything; the medians of the repeats are reported.  --out writes the JSON."""
import argparse
import json
import os
import sys
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dynamic-visual-slam_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def measure(cols, rows, nfeatures, frames_n, warmup, repeats, f=600.0, z0=1.5):
    import replay_tracking as rt
    from dvslam_amd import synth, tracker as T
    frames = [synth.make_traj_frame(t, cols, rows) for t in range(frames_n)]
    depth = rt.make_depth(rows, cols, z0)
    trackers = {"fm_cv": T.Tracker(T.default_params(rows, cols, f, f, cols / 2.0, rows / 2.0, nfeatures=nfeatures, fm_mode=1)),
                "fm_own": T.Tracker(T.default_params(rows, cols, f, f, cols / 2.0, rows / 2.0, nfeatures=nfeatures))}
    stages = rt.HipStages(nfeatures)
    per = {k: [] for k in list(trackers) + ["loop"]}
    keyframes = {}
    for rep in range(repeats + 1):                       # repetition 0 is the warm-up (first `warmup` frames only)
        n = warmup if rep == 0 else frames_n
        for name, tr in trackers.items():
            tr.reset()
            t0 = time.perf_counter()
            kf = 0
            for t in range(n):
                r, _ = tr.track(frames[t], depth, (t, 0))
                kf += r["is_keyframe"]
            dt = time.perf_counter() - t0
            if rep:
                per[name].append(1e3 * dt / n); keyframes[name] = kf
        res = rt.track(stages, n, cols, rows, f, z0, nfeatures, ba_every=0, frames=frames[:n])
        if rep:
            per["loop"].append(1e3 * res["seconds_in_stages"] / n)
    for tr in trackers.values():
        tr.close()
    med = {k: float(np.median(v)) for k, v in per.items()}
    return dict(resolution=[cols, rows], nfeatures=nfeatures, frames=frames_n, warmup_frames=warmup, repeats=repeats, keyframes=keyframes,
                one_stage_loop_ms_per_frame=med["loop"], tracker_fm_cv_ms_per_frame=med["fm_cv"], tracker_fm_own_ms_per_frame=med["fm_own"],
                ratio_loop_over_tracker_fm_cv=med["loop"] / med["fm_cv"], ratio_loop_over_tracker_fm_own=med["loop"] / med["fm_own"], all_runs=per)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch  # noqa: F401  (one ROCm stack per process: tests/conftest.py)
    out = dict(what="wall milliseconds per frame, median of the repeats: dvs_tracker_track (fm_cv: fm_mode = 1, the loop's estimators; fm_own: the "
                    "defaults) against replay_tracking.track(HipStages, pre=None), whose time includes its Python culling and numpy glue",
               configs=[measure(640, 480, 1000, a.frames, a.warmup, a.repeats), measure(1280, 720, 2000, a.frames, a.warmup, a.repeats)])
    print(json.dumps(out, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(out, open(a.out, "w"), indent=1)
