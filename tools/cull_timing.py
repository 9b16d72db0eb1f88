"""Times keyframe culling on the mapping backend (csrc/kf_cull.hip) on one GPU.
    python tools/cull_timing.py [--reps 20] [--apply-reps 3] [--out FILE.json]      wall times
    python tools/cull_timing.py --mode profile --dir DIR [--out FILE.json]          per-kernel times of dry runs: starts
                                                                                    `rocprofv3 --kernel-trace --stats` on --mode kernels
Maps, those of tools/covisibility_timing.py (built through dvs_backend_add_keyframe, exact projections, every world point its own random
descriptor, so the association follows the geometry):
  full     64 keyframes x 2000 landmarks, every keyframe sees every landmark
  banded   1024 keyframes x 3072 landmarks along a corridor, the camera stepping 0.2 m: a landmark is seen by about 25 keyframes
Wall figures are ms of a blocking call, the median (min .. max) of `reps` calls after two warm-up calls:
  dry_run        MappingBackend.cull_keyframes(apply=False) with the defaults: covis_prepare, the counts, the walk, the apply's flags
  dry_run_1      the same with max_cull=1: the walk stops at its first cull, everything else is the same launches
  dry_run_local  local scope around the newest keyframe: one row of weights more
  graph_lists    MappingBackend.covisibility(15, weights=False) on the same handle: it shares covis_prepare
  apply          MappingBackend.cull_keyframes() with the defaults on a freshly built map, `apply_reps` maps (an apply changes the map);
                 followed by what a second call on the culled map costs (it culls nothing)
The share of the sequential walk is k_cull_walk's time over the sum of all kernels of a dry run, from the profile mode.
No time is promised for any of them; EXPERIMENTS.md "Keyframe culling" says what has been run."""
import argparse
import glob
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dynamic-visual-slam_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from covisibility_timing import FX, FY, CX, CY, keyframes, stats, timed    # noqa: E402

PROFILE_DRY_RUNS = 20


def build(shape):
    from dvslam_amd.backend import MappingBackend
    mb = MappingBackend(FX, FY, CX, CY, filtered=())
    newest = None
    for kf in keyframes(shape):
        mb.add_keyframe(kf["frame_id"], kf["stamp"], kf["t"], kf["q"], kf["xyz"], kf["px"], kf["desc"])
        newest = kf["frame_id"]
    return mb, newest


def mode_wall(reps, apply_reps):
    res = {"clock": "wall, blocking calls", "reps": reps, "apply_reps": apply_reps, "maps": []}
    for shape in ("full", "banded"):
        mb, newest = build(shape)
        c = mb.counts()
        rep = mb.cull_keyframes(apply=False)
        loc = mb.cull_keyframes(newest, apply=False)
        row = {"shape": shape, "keyframes": c["n_keyframes"], "landmarks": c["n_landmarks"], "observations": c["n_observations"],
               "report": {k: v for k, v in rep.items() if isinstance(v, int)}, "local_report": {k: v for k, v in loc.items() if isinstance(v, int)}}
        row["dry_run"] = timed(reps, lambda: mb.cull_keyframes(apply=False))
        row["dry_run_1"] = timed(reps, lambda: mb.cull_keyframes(apply=False, max_cull=1))
        row["dry_run_local"] = timed(reps, lambda: mb.cull_keyframes(newest, apply=False))
        row["graph_lists"] = timed(reps, lambda: mb.covisibility(15, weights=False))
        mb.close()
        ms, again = [], []
        for _ in range(apply_reps):
            mb, _ = build(shape)
            mb.cull_keyframes(apply=False)                                   # warm: the scratch is sized, the code objects are loaded
            t0 = time.perf_counter(); got = mb.cull_keyframes(); t1 = time.perf_counter()
            assert got["n_culled"] == rep["n_culled"] and mb.counts()["n_keyframes"] == c["n_keyframes"] - rep["n_culled"]
            ms.append((t1 - t0) * 1e3)
            t0 = time.perf_counter(); got = mb.cull_keyframes(); t1 = time.perf_counter()
            again.append((t1 - t0) * 1e3)
            row["second_call_culled"] = got["n_culled"]
            mb.close()
        row["apply"] = stats(ms); row["apply_second_call"] = stats(again)
        res["maps"].append(row)
        print(json.dumps(row), flush=True)
    return res


def mode_kernels():
    """what the profile traces: PROFILE_DRY_RUNS default dry runs on the banded map, after the map is built"""
    mb, _ = build("banded")
    for _ in range(PROFILE_DRY_RUNS):
        rep = mb.cull_keyframes(apply=False)
    mb.close()
    return {"dry_runs": PROFILE_DRY_RUNS, "n_culled": rep["n_culled"]}


def mode_profile(out_dir):
    import csv
    os.makedirs(out_dir, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out_dir, "-o", "cull", "--", sys.executable, os.path.abspath(__file__), "--mode", "kernels"]
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=560)
    if run.returncode != 0:
        raise SystemExit(f"rocprofv3 failed ({run.returncode}):\n{run.stdout[-2000:]}\n{run.stderr[-2000:]}")
    files = glob.glob(os.path.join(out_dir, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no kernel statistics under {out_dir}")
    # the kernels only the dry runs launch; the views CSR's kernels and the scans also serve the map's construction and cannot be told apart by name
    mine =("k_cull_", "k_covis_first", "k_covis_scatter", "k_covis_order", "k_compact_")
    rows = []
    for r in csv.DictReader(open(files[0])):
        name = r.get("Name", "").split("(")[0]
        if any(k in name for k in mine):
            rows.append({"kernel": name, "calls": int(r["Calls"]), "average_us": round(float(r["AverageNs"]) / 1e3, 2), "min_us": round(float(r["MinNs"]) / 1e3, 2),
                         "max_us": round(float(r["MaxNs"]) / 1e3, 2)})
    per_run = sum(r["average_us"] * r["calls"] for r in rows) / PROFILE_DRY_RUNS
    walk = sum(r["average_us"] * r["calls"] for r in rows if "k_cull_walk" in r["kernel"] and "gather" not in r["kernel"]) / PROFILE_DRY_RUNS
    return {"shape": "banded", "dry_runs": PROFILE_DRY_RUNS, "source": os.path.relpath(files[0], out_dir), "kernels": rows,
            "note": "kernels of the dry runs that kf_cull.hip and covis_prepare's own part launch; the views CSR's kernels and the scans also serve add_keyframe and are left out",
            "listed_kernel_us_per_dry_run": round(per_run, 2), "walk_us_per_dry_run": round(walk, 2), "walk_share_of_listed": round(walk / per_run, 4) if per_run else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("wall", "kernels", "profile"), default="wall")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--apply-reps", type=int, default=3)
    ap.add_argument("--dir", default="cull_profile")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = mode_wall(a.reps, a.apply_reps) if a.mode == "wall" else mode_kernels() if a.mode == "kernels" else mode_profile(a.dir)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
