#!/usr/bin/env python3
"""Times the motion segmentation (csrc/motion_seg.hip) on one GPU.  Three measurements, each a mode of its own:
    python tools/motion_timing.py --mode profile --dir DIR   per-kernel times: starts `rocprofv3 --kernel-trace --stats` (no counters in the
                                                             run) on a fresh child running --mode kernels and prints the rows of its
                                                             kernel statistics that belong to a dvs_motion_segment_device call
    python tools/motion_timing.py --mode kernels             what that child runs: 50 calls at 1280 x 720 after 5 warm-up calls
    python tools/motion_timing.py --mode events              device-event time of ONE dvs_motion_segment_device call at 1280 x 720 (events
                                                             recorded on the handle's stream either side of the call): median, min, max
                                                             over --reps calls after warm-up, for a static pair (no seed) and for a pair
                                                             with a moving block (one component of 19 200 pixels)
    python tools/motion_timing.py --mode tracker             wall milliseconds per dvs_tracker_track call at 640 x 480 with the motion mask
                                                             on (lag 4) and off: two trackers in one process over the same frames, taking
                                                             turns repetition by repetition; medians of the repetitions
No time is promised for any of them; EXPERIMENTS.md "Motion segmentation" says what has been run.  --out appends the JSON line to a file."""
import argparse
import glob
import json
import os
import statistics
import subprocess
import sys
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dynamic-visual-slam_amd"))
KERNELS = ("k_seed", "k_label_tile", "k_merge_borders", "k_flatten_count", "k_dynamic_hdilate", "k_vdilate_mask")
COLS, ROWS, F = 1280, 720, 900.0


def stats(ms):
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def pair(block):
    """reference: a wall at 1.5 m; current: the same seen 30 mm to the side, with a 160 x 120 px block at 0.9 m when asked"""
    ref = np.full((ROWS, COLS), 1500, np.uint16)
    cur = ref.copy()
    if block:
        cur[300:420, 500:660] = 900
    return ref, cur, np.eye(3), np.array([0.03, 0.0, 0.0])


class Setup:
    def __init__(self):
        from dvslam_amd import motion as M, stream_create
        from dvslam_amd._lib import DeviceBuffer
        self.seg = M.MotionSegmenter(M.default_params(ROWS, COLS, F, F, COLS / 2.0, ROWS / 2.0))
        self.stream = stream_create()
        self.seg.set_stream(self.stream)
        self.d_ref, self.d_cur, self.d_mask = DeviceBuffer(ROWS * COLS * 2), DeviceBuffer(ROWS * COLS * 2), DeviceBuffer(ROWS * COLS)

    def load(self, block):
        ref, cur, self.R, self.t = pair(block)
        self.d_ref.upload(ref); self.d_cur.upload(cur)

    def call(self, want_stats=False):
        return self.seg.segment_device(self.d_ref, COLS * 2, self.d_cur, COLS * 2, self.R, self.t, self.d_mask, COLS, want_stats=want_stats)


def mode_kernels():
    from dvslam_amd._lib import stream_synchronize
    s = Setup()
    s.load(True)
    for _ in range(55):
        s.call()
    stream_synchronize(s.stream)
    return {"calls": 55, "stats": s.call(True)}


def mode_profile(out_dir):
    os.makedirs(out_dir, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out_dir, "-o", "motion", "--", sys.executable, os.path.abspath(__file__),
           "--mode", "kernels"]
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=280)
    if run.returncode != 0:
        raise SystemExit(f"rocprofv3 failed ({run.returncode}):\n{run.stdout[-2000:]}\n{run.stderr[-2000:]}")
    files = glob.glob(os.path.join(out_dir, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no kernel statistics under {out_dir}")
    import csv
    rows = []
    for r in csv.DictReader(open(files[0])):
        if any(k in r.get("Name", "") for k in KERNELS):
            rows.append({"kernel": r["Name"].split("(")[0], "calls": int(r["Calls"]), "average_us": round(float(r["AverageNs"]) / 1e3, 2),
                         "min_us": round(float(r["MinNs"]) / 1e3, 2), "max_us": round(float(r["MaxNs"]) / 1e3, 2)})
    return {"resolution": [COLS, ROWS], "scene": "wall and moving block", "source": os.path.relpath(files[0], out_dir), "kernels": rows,
            "sum_of_averages_us": round(sum(r["average_us"] for r in rows), 2)}


def mode_events(reps):
    from dvslam_amd import lib
    from dvslam_amd._lib import stream_synchronize
    from dvslam_amd._lib import timing_event_create, event_elapsed_ms, check
    L = lib()
    s = Setup()
    a, b = timing_event_create(), timing_event_create()
    out = {"resolution": [COLS, ROWS], "reps": reps, "clock": "device events on the handle's stream around one dvs_motion_segment_device call"}
    for name, block in (("static", False), ("moving_block", True)):
        s.load(block)
        ms = []
        for rep in range(reps + 10):
            check(L.dvs_event_record(a, s.stream))
            s.call()
            check(L.dvs_event_record(b, s.stream))
            stream_synchronize(s.stream)
            if rep >= 10:
                ms.append(event_elapsed_ms(a, b))
        out[name] = {"ms": stats(ms), "stats": s.call(True)}
    return out


def mode_tracker(frames_n, reps):
    from dvslam_amd import synth, tracker as T, motion as M
    cols, rows, f = 640, 480, 600.0
    frames = [synth.make_traj_frame(t, cols, rows) for t in range(frames_n)]
    depth = np.full((rows, cols), 1500, np.uint16)
    tr = {k: T.Tracker(T.default_params(rows, cols, f, f, cols / 2.0, rows / 2.0)) for k in ("off", "on")}
    tr["on"].set_motion_mask(M.default_params(), 4)
    per = {"off": [], "on": []}
    for rep in range(reps + 1):                          # repetition 0 warms up
        for name in (("off", "on") if rep % 2 else ("on", "off")):
            tr[name].reset()
            t0 = time.perf_counter()
            for t in range(frames_n):
                tr[name].track(frames[t], depth, (t, 0), want_payload=False)
            if rep:
                per[name].append(1e3 * (time.perf_counter() - t0) / frames_n)
    for t in tr.values():
        t.close()
    return {"resolution": [cols, rows], "frames": frames_n, "reps": reps, "clock": "wall per dvs_tracker_track call, static scene, lag 4",
            "off_ms_per_frame": stats(per["off"]), "on_ms_per_frame": stats(per["on"]),
            "difference_of_medians_ms": round(statistics.median(per["on"]) - statistics.median(per["off"]), 4)}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["profile", "kernels", "events", "tracker"], required=True)
    ap.add_argument("--dir", default="motion_profile")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.mode != "profile":
        import torch  # noqa: F401  (one ROCm stack per process: tests/conftest.py)
    res = {"mode": a.mode}
    res.update(mode_profile(a.dir) if a.mode == "profile" else mode_kernels() if a.mode == "kernels" else mode_events(a.reps) if a.mode == "events"
               else mode_tracker(a.frames, min(a.reps, 7)))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write(line + "\n")
