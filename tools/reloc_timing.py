#!/usr/bin/env python3
"""Times the relocalisation (csrc/reloc.hip) on one GPU: 2000 keypoints at 640 x 480 against 20 000 and 200 000 landmarks.
    python tools/reloc_timing.py [--reps 50] [--out FILE]
Per map size, over --reps calls after 10 warm-up calls (median, min, max):
    call_ms      wall around one dvs_reloc_locate_device call (stages 1-5; the call ends in two waits, its own and the confirmation's)
    stage1_ms    device events on the handle's stream (dvs_reloc_set_timing): the matrix-core top-2 and the proposals
    stage23_ms   the same: the one-to-one assignment's list
    stage4_ms    the same: P3P RANSAC and the record's export
    stage5_ms    wall around a separate dvs_maptrack_track_device call with the found pose as the prior (it runs on the map tracker's stream)
No time is promised for any of them; EXPERIMENTS.md "Relocalisation" says what has been run.  --out appends the JSON line to a file."""
import argparse
import json
import os
import statistics
import sys
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dynamic-visual-slam_amd"))
COLS, ROWS, F, N_KP = 640, 480, 520.0, 2000


def stats(ms):
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def scene(n_lm, n_kp=N_KP, seed=1):
    """landmarks all round a camera that looks back over its shoulder (150 degrees from the identity, 2 m away); a keypoint with a half-pixel
    error and a few flipped descriptor bits on up to 0.7 n_kp of the visible ones, the rest of the keypoints random"""
    from dvslam_amd._lib import KP_DTYPE
    rng = np.random.default_rng(seed)
    a = np.radians(150.0)
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]); t = np.array([1.0, 0.2, -1.7])
    xyz = np.stack([rng.uniform(-8, 8, n_lm), rng.uniform(-3, 3, n_lm), rng.uniform(-8, 8, n_lm)], 1).astype(np.float32)
    c = (xyz.astype(np.float64) - t) @ R
    with np.errstate(divide="ignore", invalid="ignore"):
        u = F * c[:, 0] / c[:, 2] + COLS / 2.0; v = F * c[:, 1] / c[:, 2] + ROWS / 2.0
    vis = np.flatnonzero((c[:, 2] > 0.5) & (c[:, 2] < 15) & (u >= 8) & (u < COLS - 8) & (v >= 8) & (v < ROWS - 8))
    pick = rng.choice(vis, min(int(0.7 * n_kp), len(vis)), replace=False)
    ldesc = rng.integers(0, 256, (n_lm, 32), dtype=np.uint8)
    kdesc = rng.integers(0, 256, (n_kp, 32), dtype=np.uint8)
    kdesc[:len(pick)] = ldesc[pick]
    flip = rng.integers(0, 256, (len(pick), 6))
    for col in range(6):
        kdesc[np.arange(len(pick)), flip[:, col] >> 3] ^= (1 << (flip[:, col] & 7)).astype(np.uint8)
    kps = np.zeros(n_kp, KP_DTYPE)
    kps["x"] = rng.uniform(8, COLS - 8, n_kp); kps["y"] = rng.uniform(8, ROWS - 8, n_kp)
    kps["x"][:len(pick)] = u[pick] + rng.normal(0, 0.5, len(pick)); kps["y"][:len(pick)] = v[pick] + rng.normal(0, 0.5, len(pick))
    kps["octave"] = rng.integers(0, 8, n_kp); kps["size"] = 31.0; kps["class_id"] = -1
    return dict(xyz=xyz, ldesc=ldesc, ids=np.arange(n_lm, dtype=np.int64), kps=kps, kdesc=kdesc, R=R, t=t, in_view=int(len(vis)), true_pairs=int(len(pick)))


def run(reps):
    from dvslam_amd import map_track as M, reloc as RL, stream_create
    from dvslam_amd._lib import DeviceBuffer
    out = {"resolution": [COLS, ROWS], "keypoints": N_KP, "reps": reps}
    for n_lm in (20000, 200000):
        s = scene(n_lm)
        mt = M.MapTracker(M.default_params(ROWS, COLS, F, F, COLS / 2.0, ROWS / 2.0))
        rl = RL.Relocalizer(RL.default_params(F, F, COLS / 2.0, ROWS / 2.0))
        stream = stream_create()
        rl.set_stream(stream)
        rl.set_timing(True)
        bufs = [DeviceBuffer(s[k].nbytes).upload(s[k]) for k in ("xyz", "ldesc", "ids", "kps", "kdesc")]
        args = (bufs[0], bufs[1], bufs[2], n_lm, bufs[3], bufs[4], N_KP)
        call, st1, st23, st4, st5 = [], [], [], [], []
        for rep in range(reps + 10):
            t0 = time.perf_counter()
            res = rl.locate_device(mt, *args)
            t1 = time.perf_counter()
            ms = rl.stage_ms()
            t2 = time.perf_counter()
            if res["status"] in (RL.OK, RL.NOT_CONFIRMED):
                mt.track_device(*args, res["pnp_R"], res["pnp_t"])
            t3 = time.perf_counter()
            if rep >= 10:
                call.append(1e3 * (t1 - t0)); st1.append(ms["stage1"]); st23.append(ms["stage23"]); st4.append(ms["stage4"]); st5.append(1e3 * (t3 - t2))
        err = float(max(np.abs(res["R"] - s["R"]).max(), np.abs(res["t"] - s["t"]).max()))
        out[f"landmarks_{n_lm}"] = {"call_ms": stats(call), "stage1_ms": stats(st1), "stage23_ms": stats(st23), "stage4_ms": stats(st4), "stage5_ms": stats(st5),
                                    "in_view": s["in_view"], "true_pairs": s["true_pairs"], "pose_error": err,
                                    "result": {k: res[k] for k in RL.RelocResult.INT_FIELDS}, "track_inliers": res["track"]["n_inliers"]}
        for b in bufs:
            b.free()
        rl.close(); mt.close()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch  # noqa: F401  (one ROCm stack per process: tests/conftest.py)
    res = run(a.reps)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write(line + "\n")
