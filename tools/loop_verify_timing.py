"""Times loop verification (csrc/loop_verify.hip) on one GPU: one 2000-row query keyframe against a database of 64 keyframes, the top 4
candidates verified.
    python tools/loop_verify_timing.py [--reps 20] [--rounds 5] [--out FILE.json]
Two paths on the same inputs, both from host descriptors and points to a relative pose per candidate, both timed as WALL time per call
(each call blocks until its results are on the host), after 3 warm-up calls, `rounds` windows of `reps` calls, median (min .. max) in ms:
  detect_verify   LoopDatabase.detect_verify: transform, query, guided match and the rigid 3D-3D verification in one enqueue, one read-back
  detect_gather_pnp  what a caller had before: LoopDatabase.detect, a host gather of (entry point, query pixel) pairs from train_idx,
                  FrontendGlue.solve_pnp_ransac_batch (dvs_solve_pnp_ransac_batch imports the lists again)
The scene: every keyframe sees 2000 points of one synthetic room (K = 615, 615, 320, 240) from a pose of its own; the query is keyframe
10's place seen again under a small motion with 0.5 px / 0.2 % depth noise and 1/16 of its descriptor bits flipped.  Descriptors are
random per 3D point, so matches are correct up to the guided match's own mistakes.  The two paths estimate different models (3D-3D
against 3D-2D), so their poses are reported, not compared.  No time is promised for either."""
import argparse
import json
import os
import statistics
import sys
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dynamic-visual-slam_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
K4 = (615.0, 615.0, 320.0, 240.0)


def rot(axis, angle):
    a = np.asarray(axis, np.float64); a /= np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * Kx @ Kx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from bow_timing import full_tree
    from dvslam_amd import OrbVocabulary, LoopDatabase, LoopVerifyParams
    from dvslam_amd.glue import FrontendGlue
    k, L, rows, levels, places, top = 10, 6, 2000, 4, 64, 4
    parent, leaf, desc, weight = full_tree(k, L, 1)
    voc = OrbVocabulary.from_arrays(k, L, parent, leaf, desc, weight)
    rng = np.random.Generator(np.random.PCG64(4))

    def seen_again(block):
        noise = rng.integers(0, 256, block.shape, dtype=np.uint8)
        for _ in range(3):
            noise &= rng.integers(0, 256, block.shape, dtype=np.uint8)
        return block ^ noise

    def cloud(n):
        uv = np.stack([rng.uniform(20, 620, n), rng.uniform(20, 460, n)], 1)
        z = rng.uniform(0.6, 6.0, n)
        return np.stack([(uv[:, 0] - K4[2]) * z / K4[0], (uv[:, 1] - K4[3]) * z / K4[1], z], 1)

    db = LoopDatabase(voc, levels)
    host_desc = rng.integers(0, 256, (places, rows, 32), dtype=np.uint8)
    host_xyz = [cloud(rows) for _ in range(places)]
    for f in range(places):
        db.set_points(db.add(host_desc[f]), host_xyz[f].astype(np.float32))
    R, t = rot([0.3, 1.0, -0.2], 0.2), np.array([0.25, -0.05, 0.15])
    xq = host_xyz[10] @ R.T + t
    uv = np.stack([K4[0] * xq[:, 0] / xq[:, 2] + K4[2], K4[1] * xq[:, 1] / xq[:, 2] + K4[3]], 1) + rng.normal(0, 0.5, (rows, 2))
    zq = xq[:, 2] * (1 + rng.normal(0, 0.002, rows))
    q_xyz = np.stack([(uv[:, 0] - K4[2]) * zq / K4[0], (uv[:, 1] - K4[3]) * zq / K4[1], zq], 1).astype(np.float32)
    q_uv = uv.astype(np.float32)
    q_desc = seen_again(host_desc[10])
    P = LoopVerifyParams(K4)
    glue = FrontendGlue()
    entry_xyz = [p.astype(np.float32) for p in host_xyz]

    def one_call():
        return db.detect_verify(q_desc, q_xyz, P, top)

    def old_path():
        ids, scores, nm, train, dist = db.detect(q_desc, top)
        objs, imgs = [], []
        for c, e in enumerate(ids):
            m = train[c] >= 0
            objs.append(entry_xyz[int(e)][train[c][m]]); imgs.append(q_uv[m])
        return ids, glue.solve_pnp_ransac_batch(objs, imgs, K4, [1] * len(ids), 256, 4.0, 0.99)

    def timed(fn):
        for _ in range(3):
            fn()
        out = []
        for _ in range(a.rounds):
            t0 = time.perf_counter()
            for _ in range(a.reps):
                fn()
            out.append((time.perf_counter() - t0) * 1e3 / a.reps)
        return {"median": round(statistics.median(out), 4), "min": round(min(out), 4), "max": round(max(out), 4)}

    res = {"shape": {"k": k, "L": L, "rows": rows, "di_levels": levels, "entries": db.size(), "top": top, "iterations": 256, "reps": a.reps,
                     "rounds": a.rounds, "clock": "wall, blocking calls"}}
    res["detect_verify_ms"] = timed(one_call)
    res["detect_gather_pnp_ms"] = timed(old_path)
    ids, scores, nm, train, dist, rec, mask = one_call()
    res["candidates"] = ids.tolist(); res["n_matches"] = nm.tolist()
    res["verify"] = [{"n_corr": int(r["n_corr"]), "n_inliers": int(r["n_inliers"]), "success": int(r["success"]), "iterations": int(r["iterations"]),
                      "rms_px": round(float(r["rms_px"]), 4), "t_err_m": round(float(np.linalg.norm(r["tvec"] - t)), 6)} for r in rec]
    ids2, pnp = old_path()
    res["pnp"] = [{"success": bool(ok), "n_inliers": int(len(inl)), "t_err_m": round(float(np.linalg.norm(tv - t)), 6)} for ok, rv, tv, inl in pnp]
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
