"""Times loop closing on the map (csrc/loop_close.hip, dvs_backend_close_loop / dvs_backend_fuse) on one GPU.
    python tools/loop_close_timing.py [--keyframes 200] [--obs 2000] [--entries 42] [--reps 5] [--out FILE.json]
The map: a camera that goes out along a corridor and comes back beside it (`keyframes` keyframes, about `obs` observations each, one
class), reported with a translation drift that grows to 0.2 m; the last keyframe stands at the start again and, 40 pixels off, creates
duplicates of the first keyframes' landmarks.  The loop edge is the true relative pose of the last keyframe against the first.
Every figure is WALL time of blocking calls (each ends in a stream synchronisation), the median (min .. max) of `reps` calls after a
warm-up on a 12-keyframe map that loads the code objects, in ms.  Between the repetitions the poses and positions are put back through
dvs_backend_apply_optimized (not timed), and the two paths alternate:
  device path   anchors        dvs_backend_get_anchors (views CSR, anchors, read-back of ids and anchors)
                graph          dvs_backend_build_pose_graph (host only)
                close          dvs_backend_close_loop without fusion, the whole call
                solve          of it: dvs_pgo_set_nodes + set_edges + solve, measured on a second handle from the same start
                correction     of it: dvs_pgo_correct_points_device on the landmark count, measured on a device copy
                write-back     the remainder close - solve - correction (graph, poses up, views CSR, anchors, counts)
  host path     the same close on the entry points that existed before: the three getters, anchors and graph in numpy, the solve,
                dvs_pgo_correct_points on the host arrays, dvs_backend_apply_optimized; with its parts
  fusion        dvs_backend_fuse with q = the last keyframe and E = the first `entries` keyframes: `reps` dry runs, then ONE applied run
                (it changes the map; a single sample).  Kernel times per stage (k_fuse_mark, _lists, _propose, _resolve, _pairs,
                _pairlist, _repoint, _compact) come from a kernel trace of this tool, taken in a run of its own.
No time is promised for any of them; EXPERIMENTS.md "Loop closing" says what has been run."""
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

FX = FY = 600.0; CX, CY = 320.0, 240.0
Z180 = (0.0, 0.0, 1.0, 0.0)
LANE = 2.6
DRIFT = np.array([0.19, 0.06, 0.0])


def stats(ms):
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def make_map(nkf, obs, seed=1):
    """keyframes as tests/loop_closing_ref.make_scene's, at any size; descriptor noise is vectorised (up to 10 bit flips, repeats allowed)"""
    rng = np.random.default_rng(seed)
    half = nkf // 2
    step = 0.3
    pos = [(step * k, 0.0) for k in range(half)] + [(step * (nkf - 2 - k), LANE) for k in range(half, nkf - 1)] + [(0.05, 0.02)]
    T = np.array([(x, y, 0.0) for x, y in pos])
    x0, x1, y0, y1 = -1.7, step * half + 1.7, -1.3, LANE + 1.3
    npts = int(obs / (3.2 * 2.4) * (x1 - x0) * (y1 - y0))
    X = np.stack([rng.uniform(x0, x1, npts), rng.uniform(y0, y1, npts), rng.uniform(2.6, 3.4, npts)], 1)
    D = rng.integers(0, 256, (npts, 32), dtype=np.uint8)
    out = []
    for k in range(nkf):
        t = T[k]
        xc = np.stack([-(X[:, 0] - t[0]), -(X[:, 1] - t[1]), X[:, 2]], 1)
        u = FX * xc[:, 0] / xc[:, 2] + CX; v = FY * xc[:, 1] / xc[:, 2] + CY
        vis = np.nonzero((u > 8) & (u < 632) & (v > 8) & (v < 472))[0]
        vis = vis[rng.permutation(len(vis))]
        n = len(vis)
        px = np.stack([u[vis], v[vis]], 1) + rng.normal(0, 0.3, (n, 2))
        desc = D[vis].copy()
        bits = rng.integers(0, 256, (n, 10)); use = rng.integers(0, 11, n)[:, None] > np.arange(10)[None, :]
        rows = np.arange(n)
        for c in range(10):
            desc[rows, bits[:, c] >> 3] ^= ((1 << (bits[:, c] & 7)) * use[:, c]).astype(np.uint8)
        drift = DRIFT * (k / (nkf - 1))
        out.append(dict(frame_id=1000 + k, stamp=(10 + k, 0), t=t + drift, q=Z180, xyz=X[vis] + drift + rng.normal(0, 0.01, (n, 3)), px=px, desc=desc))
    tvec = np.array([-(T[0][0] - T[-1][0]), -(T[0][1] - T[-1][1]), 0.0])      # R^T (t_0 - t_last) with R = diag(-1, -1, 1)
    return out, [(1000 + nkf - 1, 1000, (0.0, 0.0, 0.0), tvec, 300.0, 200.0)]


def build(scene, **kw):
    from dvslam_amd.backend import MappingBackend
    mb = MappingBackend(FX, FY, CX, CY, filtered=(), **kw)
    for kf in scene:
        mb.add_keyframe(kf["frame_id"], kf["stamp"], kf["t"], kf["q"], kf["xyz"], kf["px"], kf["desc"], [])
    return mb


def so3_log_rows(Q):
    v = np.stack([Q[:, 2, 1] - Q[:, 1, 2], Q[:, 0, 2] - Q[:, 2, 0], Q[:, 1, 0] - Q[:, 0, 1]], 1) / 2
    s = np.sqrt((v * v).sum(1)); c = (Q[:, 0, 0] + Q[:, 1, 1] + Q[:, 2, 2] - 1) / 2
    k = np.where(s > 1e-12, np.arctan2(s, c) / np.where(s > 1e-12, s, 1.0), 1.0)
    return v * k[:, None]


def host_close(mb, pg, loops, odo, ms):
    """the close on the entry points that existed before dvs_backend_close_loop; appends the parts' times to ms"""
    t0 = time.perf_counter()
    L, O, K = mb.landmarks(), mb.observations(), mb.keyframes()
    t1 = time.perf_counter()
    kf_of = {int(f): k for k, f in enumerate(K["frame_id"])}
    lm, first = np.unique(O["landmark_id"], return_index=True)          # the table is in ascending observation id
    obs_kf = np.searchsorted(K["frame_id"], O["frame_id"][first]).astype(np.int32)      # this tool's frame ids ascend with the keyframe index
    anc = np.full(len(L["id"]), -1, np.int32)
    anc[np.searchsorted(L["id"], lm)] = obs_kf
    R, t = K["R"], K["t"]
    Rz = np.einsum("nkr,nkc->nrc", R[:-1], R[1:]); tz = np.einsum("nkr,nk->nr", R[:-1], t[1:] - t[:-1])
    n = len(R)
    ei = np.concatenate([np.arange(n - 1), [kf_of[l[0]] for l in loops]]).astype(np.int32)
    ej = np.concatenate([np.arange(1, n), [kf_of[l[1]] for l in loops]]).astype(np.int32)
    rv = np.concatenate([so3_log_rows(Rz), np.array([l[2] for l in loops], np.float64).reshape(-1, 3)])
    tv = np.concatenate([tz, np.array([l[3] for l in loops], np.float64).reshape(-1, 3)])
    wr = np.concatenate([np.full(n - 1, odo[0]), [l[4] for l in loops]]); wt = np.concatenate([np.full(n - 1, odo[1]), [l[5] for l in loops]])
    fixed = np.zeros(n, np.uint8); fixed[0] = 1
    t2 = time.perf_counter()
    pg.set_nodes(R, t, fixed).set_edges(ei, ej, rv, tv, wr, wt)
    s = pg.solve()
    t3 = time.perf_counter()
    R2, t2_ = pg.nodes()
    xyz = pg.correct_points(L["xyz"], anc)
    t4 = time.perf_counter()
    put_back(mb, K["frame_id"], R2, t2_, L["id"], L["class_id"], xyz)
    t5 = time.perf_counter()
    for k, v in (("getters", t1 - t0), ("anchors_graph_numpy", t2 - t1), ("solve", t3 - t2), ("correction_host", t4 - t3), ("apply_optimized", t5 - t4), ("total", t5 - t0)):
        ms.setdefault(k, []).append(v * 1e3)
    return s


def put_back(mb, frame_id, R, t, lm_id, lm_class, xyz):
    from dvslam_amd._lib import check, ptr
    fid = np.ascontiguousarray(frame_id, np.uint64); R = np.ascontiguousarray(R, np.float64); t = np.ascontiguousarray(t, np.float64)
    lid = np.ascontiguousarray(lm_id, np.uint64); lcl = np.ascontiguousarray(lm_class, np.int32); x = np.ascontiguousarray(xyz, np.float64)
    check(mb._L.dvs_backend_apply_optimized(mb._h, len(fid), ptr(fid), ptr(R), ptr(t), len(lid), ptr(lid), ptr(lcl), ptr(x)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, default=200)
    ap.add_argument("--obs", type=int, default=2000)
    ap.add_argument("--entries", type=int, default=42)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from dvslam_amd import PoseGraph, device_count
    from dvslam_amd._lib import DeviceBuffer
    if device_count() < 1:
        raise SystemExit("loop_close_timing needs the GPU (there is no CPU path)")
    odo = (100.0, 100.0)
    # warm-up: every entry point once on a small map
    small, sloops = make_map(12, 300, seed=2)
    w = build(small); wp = PoseGraph()
    w.anchors(); host_close(w, wp, sloops, odo, {}); w.close_loop(wp, sloops, odo, fuse={}); wp.close(); w.close()

    t0 = time.perf_counter()
    scene, loops = make_map(a.keyframes, a.obs)
    t1 = time.perf_counter()
    mb = build(scene, initial_capacity=1 << 16)
    t2 = time.perf_counter()
    c = mb.counts()
    L0, K0 = mb.landmarks(), mb.keyframes()
    res = {"clock": "wall, blocking calls", "reps": a.reps, "keyframes": c["n_keyframes"], "observations": c["n_observations"], "landmarks": c["n_landmarks"],
           "observations_per_keyframe": round(c["n_observations"] / c["n_keyframes"], 1), "scene_s": round(t1 - t0, 2), "build_map_s": round(t2 - t1, 2)}
    restore = lambda: put_back(mb, K0["frame_id"], K0["R"], K0["t"], L0["id"], L0["class_id"], L0["xyz"])
    pg, parts = PoseGraph(), PoseGraph()
    dev, host = {}, {}
    nlm = c["n_landmarks"]
    for rep in range(a.reps + 1):
        d = {}
        t0 = time.perf_counter(); ids, anc = mb.anchors(); d["anchors"] = time.perf_counter() - t0
        t0 = time.perf_counter(); g = mb.build_pose_graph(loops, odo); d["graph"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        parts.set_nodes(g["R"], g["t"], g["fixed"]).set_edges(g["ei"], g["ej"], g["rvec"], g["tvec"], g["w_rot"], g["w_trans"]); s2 = parts.solve()
        d["solve"] = time.perf_counter() - t0
        dx, da = DeviceBuffer(L0["xyz"].nbytes).upload(L0["xyz"]), DeviceBuffer(anc.nbytes).upload(anc)
        t0 = time.perf_counter(); parts.correct_points_device(nlm, dx.ptr, da.ptr); parts.synchronize(); d["correction"] = time.perf_counter() - t0
        dx.free(); da.free()
        t0 = time.perf_counter(); out = mb.close_loop(pg, loops, odo); d["close"] = time.perf_counter() - t0
        d["write_back"] = d["close"] - d["solve"] - d["correction"]
        closed = mb.landmarks()["xyz"].copy()
        restore()
        hs = host_close(mb, parts, loops, odo, host if rep else {})
        same = bool((mb.landmarks()["xyz"] == closed).all()) and hs.num_iterations == out["summary"].num_iterations
        restore()
        if rep:
            for k, v in d.items():
                dev.setdefault(k, []).append(v * 1e3)
    s = out["summary"]
    res["close"] = {"device_path_ms": {k: stats(v) for k, v in dev.items()}, "host_path_ms": {k: stats(v) for k, v in host.items()},
                    "both_paths_give_the_same_positions": same, "termination": s.termination, "trial_steps": s.num_iterations, "pcg_iterations": s.pcg_iterations,
                    "initial_cost": s.initial_cost, "final_cost": s.final_cost, "landmarks_moved": out["n_landmarks_moved"]}
    # fusion on the closed map
    mb.close_loop(pg, loops, odo)
    q = scene[-1]["frame_id"]; E = [kf["frame_id"] for kf in scene[:a.entries]]
    dry = []
    for rep in range(a.reps + 1):
        t0 = time.perf_counter(); f = mb.fuse(q, E, apply=False); t1 = time.perf_counter()
        if rep:
            dry.append((t1 - t0) * 1e3)
    t0 = time.perf_counter(); fa = mb.fuse(q, E, apply=True, pairs=False); t1 = time.perf_counter()
    res["fusion"] = {"entries": len(E), "query_observations": len(scene[-1]["px"]), "n_sources": f["n_sources"], "n_targets": f["n_targets"], "n_proposals": f["n_proposals"],
                     "n_fused": f["n_fused"], "dry_run_ms": stats(dry), "applied_ms_single_sample": round((t1 - t0) * 1e3, 4), "applied_n_fused": fa["n_fused"],
                     "landmarks_after": mb.counts()["n_landmarks"]}
    pg.close(); parts.close(); mb.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
