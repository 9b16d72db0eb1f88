"""Times global bundle adjustment (dvs_ba_solve_global, csrc/ba.hip) on one GPU against the two solvers that were there before.
    python tools/global_ba_timing.py [--keyframes 64 256 1024 4096] [--reps 3] [--host-max 256] [--out FILE.json]
Problems (dvslam_amd.synth): 64 keyframes x 2000 landmarks with full co-visibility (make_ba_problem, seed 64), and for every larger
count K the banded make_ba_banded_problem(K, 3 K, seed K, half_span 12): a landmark is seen by the 25 keyframes around it, about 75
observations per keyframe.  Every figure is WALL time of a blocking call in ms, the median (min .. max) of `reps` calls after one warm-up
call; dvs_ba_set_problem runs before every call and is not timed.
  global        dvs_ba_solve_global with the defaults (50 iterations, eta 0.1): with it the trial steps, the accepted ones, the PCG
                iterations and the costs
  pcg_iteration the marginal cost of one PCG iteration: (a solve of ONE trial step at eta 1e-8) - (the same with max_pcg_iterations 1),
                divided by the difference of their PCG iteration counts
  host          dvs_ba_solve (dense reduced camera system on the host) with the same limits, up to --host-max keyframes: its cost is
                cubic in the keyframes and its system 36 K^2 doubles, so beyond that it is not run
  device        at 64 keyframes, dvs_ba_solve_device with dvs_ba_set_device_window(63)
No time is promised for any of them; EXPERIMENTS.md "Global BA" says what has been run."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dynamic-visual-slam_amd"))


def stats(ms):
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def timed(g, P, reps, call):
    ms, s = [], None
    for rep in range(reps + 1):
        g.set_problem(P); g.synchronize()
        t0 = time.perf_counter(); s = call(); t1 = time.perf_counter()
        if rep:
            ms.append((t1 - t0) * 1e3)
    return ms, s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, nargs="+", default=[64, 256, 1024, 4096])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-max", type=int, default=256)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from dvslam_amd import BAProblem, synth
    res = {"clock": "wall, blocking calls", "reps": a.reps, "problems": []}
    for K in a.keyframes:
        P = synth.make_ba_problem(K=64, L=2000, seed=64) if K == 64 else synth.make_ba_banded_problem(K=K, L=3 * K, seed=K, half_span=12)
        g = BAProblem(P)
        row = {"keyframes": K, "landmarks": int(P["L"]), "observations": int(len(P["cam_idx"])), "shape": "full" if K == 64 else "banded"}
        ms, s = timed(g, P, a.reps, lambda: g.solve_global())
        row["global"] = {"ms": stats(ms), "termination": s.ba.termination, "trial_steps": s.ba.num_iterations, "accepted": s.ba.num_successful_steps,
                         "pcg_iterations": s.pcg_iterations, "initial_cost": s.ba.initial_cost, "final_cost": s.ba.final_cost}
        m_many, s_many = timed(g, P, a.reps, lambda: g.solve_global(max_iterations=1, eta=1e-8))
        m_one, s_one = timed(g, P, a.reps, lambda: g.solve_global(max_iterations=1, eta=1e-8, max_pcg_iterations=1))
        d = s_many.pcg_iterations - s_one.pcg_iterations
        row["pcg_iteration"] = {"ms": round((statistics.median(m_many) - statistics.median(m_one)) / d, 5) if d > 0 else None,
                                "iterations": s_many.pcg_iterations, "one_step_ms": stats(m_many), "one_step_one_iteration_ms": stats(m_one)}
        if K <= a.host_max:
            ms, s = timed(g, P, a.reps, lambda: g.solve(50, 1e-6, 1e-10, 1e-8))
            row["host"] = {"ms": stats(ms), "termination": s.termination, "trial_steps": s.num_iterations, "final_cost": s.final_cost}
        else:
            row["host"] = "not run"
        if K == 64:
            g.set_device_window(63)
            ms, s = timed(g, P, a.reps, lambda: g.solve_device(50, 1e-6, 1e-10, 1e-8))
            row["device"] = {"ms": stats(ms), "termination": s.termination, "trial_steps": s.num_iterations, "final_cost": s.final_cost}
        g.close()
        res["problems"].append(row)
        print(json.dumps(row), flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
