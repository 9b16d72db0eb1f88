#!/usr/bin/env python3
"""Times the tracking against the map (csrc/map_track.hip) on one GPU.  Three modes:
    python tools/maptrack_timing.py --mode events              one call at 640 x 480 with 2000 keypoints against 10 000 and 100 000 landmarks:
                                                               device-event time of dvs_maptrack_search_device (stages 1-3, events recorded on
                                                               the handle's stream either side of the asynchronous call) and wall time of
                                                               dvs_maptrack_track_device (stages 1-4, ends in a synchronise); and the
                                                               refinement alone, dvs_maptrack_refine_device on 500 correspondences (wall).
                                                               Median, min, max over --reps calls after 10 warm-up calls
    python tools/maptrack_timing.py --mode kernels             50 track calls at 100 000 landmarks after 5 warm-up calls
    python tools/maptrack_timing.py --mode profile --dir DIR   per-kernel times: starts `rocprofv3 --kernel-trace --stats` (no counters in the
                                                               run) on a fresh child running --mode kernels and prints the k_mt_* rows
No time is promised for any of them; EXPERIMENTS.md "Map tracking" says what has been run.  --out appends the JSON line to a file."""
import argparse
import glob
import json
import math
import os
import statistics
import subprocess
import sys
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dynamic-visual-slam_amd"))
KERNELS = ("k_mt_cells", "k_mt_scan", "k_mt_scatter", "k_mt_order", "k_mt_search", "k_mt_finalize", "k_mt_refine")
COLS, ROWS, F, N_KP = 640, 480, 520.0, 2000


def stats(ms):
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def scene(n_lm, n_kp=N_KP, seed=1):
    """landmarks in a slab around the camera (a good third of them in view), a keypoint with a half-pixel error and a few flipped descriptor bits
    on n_kp of the visible ones, the prior 0.3 degrees and 1 cm off the truth (identity)"""
    from dvslam_amd._lib import KP_DTYPE
    rng = np.random.default_rng(seed)
    xyz = np.stack([rng.uniform(-5, 5, n_lm), rng.uniform(-4, 4, n_lm), rng.uniform(2.0, 8.0, n_lm)], 1).astype(np.float32)
    u = F * xyz[:, 0] / xyz[:, 2] + COLS / 2.0; v = F * xyz[:, 1] / xyz[:, 2] + ROWS / 2.0
    vis = np.flatnonzero((u >= 8) & (u < COLS - 8) & (v >= 8) & (v < ROWS - 8))
    pick = rng.choice(vis, min(n_kp, len(vis)), replace=False)
    ldesc = rng.integers(0, 256, (n_lm, 32), dtype=np.uint8)
    kdesc = ldesc[pick].copy()
    flip = rng.integers(0, 256, (len(pick), 6))
    for c in range(6):
        kdesc[np.arange(len(pick)), flip[:, c] >> 3] ^= (1 << (flip[:, c] & 7)).astype(np.uint8)
    kps = np.zeros(len(pick), KP_DTYPE)
    kps["x"] = u[pick] + rng.normal(0, 0.5, len(pick)); kps["y"] = v[pick] + rng.normal(0, 0.5, len(pick))
    kps["octave"] = rng.integers(0, 8, len(pick)); kps["size"] = 31.0; kps["class_id"] = -1
    a = math.radians(0.3)
    R0 = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
    return dict(xyz=xyz, ldesc=ldesc, ids=np.arange(n_lm, dtype=np.int64), kps=kps, kdesc=kdesc, R0=R0, t0=np.array([0.006, -0.005, 0.006]),
                n_visible=int(len(vis)))


class Setup:
    def __init__(self, n_lm):
        from dvslam_amd import map_track as M, stream_create
        from dvslam_amd._lib import DeviceBuffer
        self.s = scene(n_lm)
        self.mt = M.MapTracker(M.default_params(ROWS, COLS, F, F, COLS / 2.0, ROWS / 2.0))
        self.stream = stream_create()
        self.mt.set_stream(self.stream)
        self.bufs = [DeviceBuffer(self.s[k].nbytes).upload(self.s[k]) for k in ("xyz", "ldesc", "ids", "kps", "kdesc")]
        self.n_lm, self.n_kp = n_lm, len(self.s["kps"])

    def args(self):
        b = self.bufs
        return (b[0], b[1], b[2], self.n_lm, b[3], b[4], self.n_kp, self.s["R0"], self.s["t0"])

    def close(self):
        for b in self.bufs:
            b.free()
        self.mt.close()


def refine_inputs(n=500, seed=2):
    rng = np.random.default_rng(seed)
    X = np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(2.5, 8.0, n)], 1)
    px = np.stack([F * X[:, 0] / X[:, 2] + COLS / 2.0, F * X[:, 1] / X[:, 2] + ROWS / 2.0], 1) + rng.normal(0, 0.6, (n, 2))
    out = rng.random(n) < 0.15
    px[out] += rng.uniform(-40, 40, (int(out.sum()), 2))
    return np.ascontiguousarray(X), np.ascontiguousarray(px), rng.integers(0, 8, n).astype(np.int32)


def mode_events(reps):
    from dvslam_amd import lib, map_track as M
    from dvslam_amd._lib import stream_synchronize, timing_event_create, event_elapsed_ms, check, DeviceBuffer
    L = lib()
    a, b = timing_event_create(), timing_event_create()
    out = {"resolution": [COLS, ROWS], "keypoints": N_KP, "reps": reps,
           "clocks": {"search_ms": "device events on the handle's stream around one dvs_maptrack_search_device call (no result asked for)",
                      "track_ms": "wall around one dvs_maptrack_track_device call (ends in a synchronise and the 128-byte read-back)",
                      "refine_ms": "wall around one dvs_maptrack_refine_device call"}}
    for n_lm in (10000, 100000):
        s = Setup(n_lm)
        search, track = [], []
        for rep in range(reps + 10):
            check(L.dvs_event_record(a, s.stream))
            s.mt.search_device(*s.args(), want_counts=False)
            check(L.dvs_event_record(b, s.stream))
            stream_synchronize(s.stream)
            t0 = time.perf_counter()
            res = s.mt.track_device(*s.args())
            t1 = time.perf_counter()
            if rep >= 10:
                search.append(event_elapsed_ms(a, b)); track.append(1e3 * (t1 - t0))
        out[f"landmarks_{n_lm}"] = {"search_ms": stats(search), "track_ms": stats(track), "in_view": s.s["n_visible"],
                                    "result": {k: res[k] for k in M.MapTrackResult.INT_FIELDS}}
        s.close()
    X, px, oc = refine_inputs()
    mt = M.MapTracker(M.default_params(ROWS, COLS, F, F, COLS / 2.0, ROWS / 2.0))
    bufs = [DeviceBuffer(v.nbytes).upload(v) for v in (X, px, oc)]
    a3 = math.radians(1.0)
    R0 = np.array([[1, 0, 0], [0, math.cos(a3), -math.sin(a3)], [0, math.sin(a3), math.cos(a3)]])
    ms = []
    for rep in range(reps + 10):
        t0 = time.perf_counter()
        res = mt.refine_device(bufs[0], bufs[1], bufs[2], len(X), R0, np.array([0.02, 0.01, -0.02]))
        if rep >= 10:
            ms.append(1e3 * (time.perf_counter() - t0))
    out["refine_500"] = {"refine_ms": stats(ms), "result": {k: res[k] for k in M.MapTrackResult.INT_FIELDS}}
    mt.close()
    return out


def mode_kernels():
    s = Setup(100000)
    for _ in range(55):
        res = s.mt.track_device(*s.args())
    s.close()
    return {"calls": 55, "status": res["status"], "n_matches": res["n_matches"], "n_inliers": res["n_inliers"]}


def mode_profile(out_dir):
    os.makedirs(out_dir, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out_dir, "-o", "maptrack", "--", sys.executable, os.path.abspath(__file__),
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
    return {"resolution": [COLS, ROWS], "keypoints": N_KP, "landmarks": 100000, "source": os.path.relpath(files[0], out_dir), "kernels": rows,
            "sum_of_averages_us": round(sum(r["average_us"] for r in rows), 2)}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["profile", "kernels", "events"], required=True)
    ap.add_argument("--dir", default="maptrack_profile")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.mode != "profile":
        import torch  # noqa: F401  (one ROCm stack per process: tests/conftest.py)
    res = {"mode": a.mode}
    res.update(mode_profile(a.dir) if a.mode == "profile" else mode_kernels() if a.mode == "kernels" else mode_events(a.reps))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write(line + "\n")
