"""Times vocabulary training (csrc/bow_train.hip, dvs_voc_train_device) on extractor output of the synthetic scenes (dvslam_amd/synth.py),
device-resident: (10, 6) on 64 and on 512 frames of up to 2000 descriptors, and (10, 3) on 64 frames.
    python tools/voc_train_timing.py [--reps 3] [--frames 64 512] [--ref] [--out FILE.json]
The training call blocks (it synchronises its stream), so each figure is the wall clock around one call, the median of `reps` calls after
one warm-up call.  Per level: the tree of depth l is the tree of depth l - 1 plus level l (the sampler does not depend on L), so level l's
time is reported as time(L = l) - time(L = l - 1), and `max_passes` as the most passes any node of levels 1..l ran.  --ref also times the
sequential restatement tests/bow_train_ref.py on the smallest case, as a size indication."""
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
ROWS = 2000


def extract_frames(nframes):
    """descriptors of nframes synthetic frames in the batch layout [nframes][ROWS][32], and their counts"""
    from dvslam_amd import ORBextractor, synth
    orb = ORBextractor(ROWS, 1.2, 8, 20, 7)
    block = np.zeros((nframes, ROWS, 32), np.uint8)
    counts = np.zeros(nframes, np.int32)
    for f in range(nframes):
        n, _, desc = orb(synth.make_frame(f, cols=640, rows=480))
        n = min(int(n), ROWS)
        block[f, :n] = np.asarray(desc, np.uint8).reshape(-1, 32)[:n]
        counts[f] = n
    return block, counts


def timed_create(d_desc, d_n, nframes, k, L, reps):
    from dvslam_amd import OrbVocabulary
    times, report = [], None
    for r in range(reps + 1):
        t = time.perf_counter()
        v = OrbVocabulary().create_device(d_desc.ptr, d_n.ptr, ROWS, nframes, k, L)
        dt = time.perf_counter() - t
        if r:
            times.append(dt * 1e3)
        report = v.train_report
        v.close()
    return statistics.median(times), report


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--frames", type=int, nargs="+", default=[64, 512])
    ap.add_argument("--ref", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from dvslam_amd._lib import DeviceBuffer
    block, counts = extract_frames(max(a.frames))
    d_desc = DeviceBuffer(block.nbytes).upload(block)
    d_n = DeviceBuffer(counts.nbytes).upload(counts)
    res = {"rows": ROWS, "reps": a.reps, "cases": []}
    for nframes, k, Lmax in [(f, 10, 6) for f in a.frames] + [(min(a.frames), 10, 3)]:
        case = {"frames": nframes, "features": int(counts[:nframes].sum()), "k": k, "L": Lmax, "levels": []}
        before = 0.0
        for L in range(1, Lmax + 1):
            ms, rep = timed_create(d_desc, d_n, nframes, k, L, a.reps)
            case["levels"].append({"level": L, "ms_through_level": round(ms, 3), "ms_level": round(ms - before, 3), "max_passes_so_far": rep["max_passes"],
                                   "nodes": rep["n_nodes"]})
            before = ms
        case["total_ms"] = round(before, 3)
        case["report"] = rep
        res["cases"].append(case)
    if a.ref:
        import bow_train_ref as bt
        n = min(a.frames)
        images = [block[f, :counts[f]] for f in range(n)]
        t = time.perf_counter()
        bt.train(np.concatenate(images), 10, 3)
        res["restatement_10_3_s"] = {"frames": n, "seconds": round(time.perf_counter() - t, 2)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
