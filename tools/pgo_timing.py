"""Times the pose-graph solve and the map correction (csrc/pose_graph.hip) on one GPU.
    python tools/pgo_timing.py [--nodes 300 1000 3000] [--reps 5] [--points 200000] [--out FILE.json]
Per node count N: the double-loop graph of tests/pose_graph_ref.py (odometry with 0.01 rad / 0.02 m noise, N / 100 + 2 loop edges with
0.003 rad / 0.005 m noise, node 0 fixed, initial poses chained from the odometry).  Every figure is WALL time of a blocking call, the
median (min .. max) of `reps` calls after one warm-up call, in ms:
  solve     dvs_pgo_solve with the default parameters from the same start (set_nodes before every call, not timed); with it the trial
            steps, the accepted ones, the PCG iterations and the cost before and after — times per trial step and per PCG iteration are
            quotients of these
  evaluate  dvs_pgo_evaluate (linearisation, gradient, cost, read-back of everything)
  correct   dvs_pgo_correct_points_device on `points` device-resident points with random anchors, synchronised
No time is promised for any of them; EXPERIMENTS.md "Pose graph" says what has been run."""
import argparse
import json
import os
import statistics
import sys
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dynamic-visual-slam_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def stats(ms):
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, nargs="+", default=[300, 1000, 3000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--points", type=int, default=200000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import pose_graph_ref as pr
    from dvslam_amd import PoseGraph
    from dvslam_amd._lib import DeviceBuffer
    res = {"clock": "wall, blocking calls", "reps": a.reps, "graphs": []}
    for N in a.nodes:
        loops = [(N - 1, 0), (N // 2, 1)] + [(k, k - N // 2) for k in range(N // 2 + 50, N - 1, 100)]
        g = pr.make_graph(N, loops, seed=N)
        pg = PoseGraph()
        pg.set_nodes(g.R, g.t, g.fixed).set_edges(g.ei, g.ej, g.rvec, g.tvec, g.w_rot, g.w_trans)
        solve_ms, ev_ms, s = [], [], None
        for rep in range(a.reps + 1):
            pg.set_nodes(g.R, g.t, g.fixed)
            pg.evaluate()
            t0 = time.perf_counter(); pg.evaluate(); t1 = time.perf_counter()
            s = pg.solve()
            t2 = time.perf_counter()
            if rep:
                ev_ms.append((t1 - t0) * 1e3); solve_ms.append((t2 - t1) * 1e3)
        rng = np.random.default_rng(1)
        xyz = rng.uniform(-6, 6, (a.points, 3)).astype(np.float32)
        anchor = rng.integers(0, N, a.points).astype(np.int32)
        dx, da = DeviceBuffer(xyz.nbytes).upload(xyz), DeviceBuffer(anchor.nbytes).upload(anchor)
        cor_ms = []
        for rep in range(a.reps + 1):
            t0 = time.perf_counter(); pg.correct_points_device(a.points, dx.ptr, da.ptr); pg.synchronize(); t1 = time.perf_counter()
            if rep:
                cor_ms.append((t1 - t0) * 1e3)
        dx.free(); da.free(); pg.close()
        res["graphs"].append({"nodes": N, "edges": g.E, "solve_ms": stats(solve_ms), "evaluate_ms": stats(ev_ms), "correct_ms": stats(cor_ms),
                              "points": a.points, "termination": s.termination, "trial_steps": s.num_iterations,
                              "accepted": s.num_successful_steps, "pcg_iterations": s.pcg_iterations, "initial_cost": s.initial_cost,
                              "final_cost": s.final_cost})
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
