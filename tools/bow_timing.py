"""Times the place-recognition kernels (csrc/bow.hip) on a synthetic full (10, 6) vocabulary — 1 111 110 nodes, the size of ORBvoc.txt:
the transform of 1 and of 64 frames x 2000 descriptors (device-resident), and a query against 1000 and 10 000 entries.
    python tools/bow_timing.py [--reps 20] [--out FILE.json]
Wall clock around `reps` calls enqueued back to back on the vocabulary's stream and one synchronisation (after a warm-up call)."""
import argparse
import json
import os
import sys
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dynamic-visual-slam_amd"))


def full_tree(k, L, seed):
    """breadth-first ids: level d holds k^d nodes, node i of a level is child i % k of node i // k of the level above"""
    rng = np.random.Generator(np.random.PCG64(seed))
    parent, leaf, first = [], [], 0
    for d in range(1, L + 1):
        n = k ** d
        above = first - k ** (d - 1) + 1 if d > 1 else 0          # id of the first node of the level above
        parent.append((np.arange(n) // k + above).astype(np.int32) if d > 1 else np.zeros(n, np.int32))
        leaf.append(np.full(n, 1 if d == L else 0, np.uint8))
        first += n
    parent, leaf = np.concatenate(parent), np.concatenate(leaf)
    return parent, leaf, rng.integers(0, 256, (len(parent), 32), dtype=np.uint8), rng.uniform(0.1, 9.0, len(parent))


def timed(fn, sync, reps):
    fn(); sync()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    sync()
    return (time.perf_counter() - t) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from dvslam_amd import OrbVocabulary, OrbDatabase
    from dvslam_amd._lib import DeviceBuffer
    k, L, rows, frames = 10, 6, 2000, 64
    parent, leaf, desc, weight = full_tree(k, L, 1)
    t = time.perf_counter()
    voc = OrbVocabulary.from_arrays(k, L, parent, leaf, desc, weight)
    res = {"vocabulary": {"k": k, "L": L, "nodes": int(len(parent)), "words": voc.size(), "upload_s": round(time.perf_counter() - t, 3)}}
    rng = np.random.Generator(np.random.PCG64(2))
    host = rng.integers(0, 256, (frames, rows, 32), dtype=np.uint8)
    d_desc = DeviceBuffer(host.nbytes).upload(host)
    d_n = DeviceBuffer(frames * 4).upload(np.full(frames, rows, np.int32))
    for f in (1, frames):
        ms = timed(lambda: voc.transform_batch_device(d_desc.ptr, d_n.ptr, rows, f, 0), voc.synchronize, a.reps)
        res[f"transform_{f}x{rows}_ms"] = round(ms, 4)
    res["transform_host_1x2000_ms"] = round(timed(lambda: voc.transform(host[0]), voc.synchronize, a.reps), 4)
    db = OrbDatabase(voc)
    d_ids, d_scores, d_nr = DeviceBuffer(10 * 4), DeviceBuffer(10 * 8), DeviceBuffer(4)
    for entries in (1000, 10000):
        while db.size() < entries:
            db.add_device(d_desc.ptr + (db.size() // 50 % 14) * rows * 32, d_n.ptr, rows, 50)
        voc.synchronize()
        ms = timed(lambda: db.query_device(d_desc.ptr + 63 * rows * 32, d_n.ptr, rows, 10, -1, d_ids.ptr, d_scores.ptr, 10, d_nr.ptr), voc.synchronize, a.reps)
        res[f"query_device_{entries}_entries_ms"] = round(ms, 4)
        res[f"query_host_{entries}_entries_ms"] = round(timed(lambda: db.query_arrays(host[63], 10), voc.synchronize, a.reps), 4)
        res[f"query_{entries}_results"] = int(d_nr.download(np.int32, 1)[0])
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
