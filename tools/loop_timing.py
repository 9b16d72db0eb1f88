"""Times loop-candidate detection (csrc/loop.hip) on one GPU: 2000 features per frame, a synthetic full (10, 6) vocabulary — the shape of
ORBvoc.txt — di_levels 4, 1000 entries, the top 8 candidates.
    python tools/loop_timing.py [--reps 50] [--rounds 5] [--out FILE.json]
Device events on the vocabulary's stream around `reps` calls enqueued back to back, after 3 warm-up calls; `rounds` such windows per
figure, reported as median (min .. max) in milliseconds per call.  detect_device is timed whole; its parts are timed as the calls a
caller can make — the transform alone, query_device (transform + query) and match_device (transform + match of the same 8 ids) — so
query and match are differences against the transform.  The yardstick is what a caller has without the direct index: the same 8
candidates through dvs_match_hamming_knn_batch_device (k = 2) on descriptor blocks re-supplied from the host, timed with the blocks
already resident (device time) and with their upload: that copy blocks the host, so knn2_with_upload_wall_ms is the time that passes
between the two events while the host copies and enqueues, not time the device is busy."""
import argparse
import json
import os
import statistics
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dynamic-visual-slam_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from bow_timing import full_tree
    from dvslam_amd import OrbVocabulary, LoopDatabase, BFMatcher, _lib
    from dvslam_amd._lib import DeviceBuffer, check, lib
    k, L, rows, levels, entries, top, frames = 10, 6, 2000, 4, 1000, 8, 64
    stream = _lib.stream_create()
    parent, leaf, desc, weight = full_tree(k, L, 1)
    voc = OrbVocabulary.from_arrays(k, L, parent, leaf, desc, weight, stream=stream)
    rng = np.random.Generator(np.random.PCG64(2))
    host = rng.integers(0, 256, (frames, rows, 32), dtype=np.uint8)

    def seen_again(block):
        """every bit flipped with probability 1/16 (the AND of four random bytes): about 16 bits per row"""
        noise = rng.integers(0, 256, block.shape, dtype=np.uint8)
        for _ in range(3):
            noise &= rng.integers(0, 256, block.shape, dtype=np.uint8)
        return block ^ noise

    # entry e is frame e % 64 seen again with noise of its own: the database holds each place 15 or 16 times and no two entries are equal,
    # so the top candidates of a query differ in their rows, their nodes and their matches
    batch = 50
    d_batch = DeviceBuffer(batch * rows * 32)
    d_n = DeviceBuffer(batch * 4).upload(np.full(batch, rows, np.int32))
    db = LoopDatabase(voc, levels)
    while db.size() < entries:
        d_batch.upload(seen_again(host[(db.size() + np.arange(batch)) % frames]))
        db.add_device(d_batch.ptr, d_n.ptr, rows, batch)
        voc.synchronize()                                           # the block is reused for the next batch
    q = seen_again(host[10])                                        # the query: place 10 once more
    d_q = DeviceBuffer(q.nbytes).upload(q)
    d_qn = DeviceBuffer(4).upload(np.array([rows], np.int32))
    d_ids, d_scores, d_nr, d_nm = DeviceBuffer(top * 4), DeviceBuffer(top * 8), DeviceBuffer(4), DeviceBuffer(top * 4)
    d_train, d_dist = DeviceBuffer(top * rows * 4), DeviceBuffer(top * rows * 4)
    e0, e1 = _lib.timing_event_create(), _lib.timing_event_create()

    def timed(fn):
        for _ in range(3):
            fn()
        voc.synchronize()
        out = []
        for _ in range(a.rounds):
            check(lib().dvs_event_record(e0, stream))
            for _ in range(a.reps):
                fn()
            check(lib().dvs_event_record(e1, stream))
            voc.synchronize()
            out.append(_lib.event_elapsed_ms(e0, e1) / a.reps)
        return {"median": round(statistics.median(out), 4), "min": round(min(out), 4), "max": round(max(out), 4)}

    res = {"shape": {"k": k, "L": L, "rows": rows, "di_levels": levels, "entries": db.size(), "top": top, "reps": a.reps, "rounds": a.rounds}}
    res["detect_device_ms"] = timed(lambda: db.detect_device(d_q.ptr, d_qn.ptr, rows, top, -1, d_ids.ptr, d_scores.ptr, d_nm.ptr, d_train.ptr, d_dist.ptr,
                                                            top, d_nr.ptr))
    ids = d_ids.download(np.int32, top); nm = d_nm.download(np.int32, top)
    res["candidates"] = ids.tolist(); res["n_matches"] = nm.tolist(); res["n_results"] = int(d_nr.download(np.int32, 1)[0])
    res["scores"] = [round(float(x), 4) for x in d_scores.download(np.float64, top)]
    fv = db.retrieve_features(int(ids[0]))
    res["entry_nodes"] = len(fv); res["entry_features_per_node"] = round(sum(len(x) for _, x in fv) / max(len(fv), 1), 1)
    res["transform_ms"] = timed(lambda: voc.transform_batch_device(d_q.ptr, d_qn.ptr, rows, 1, levels))
    res["query_device_ms"] = timed(lambda: db.query_device(d_q.ptr, d_qn.ptr, rows, top, -1, d_ids.ptr, d_scores.ptr, top, d_nr.ptr))
    res["match_device_ms"] = timed(lambda: db.match_device(d_q.ptr, d_qn.ptr, rows, d_ids.ptr, d_nr.ptr, top, d_train.ptr, d_dist.ptr, d_nm.ptr))
    t = res["transform_ms"]["median"]
    res["split_ms"] = {"transform": t, "query": round(res["query_device_ms"]["median"] - t, 4), "match": round(res["match_device_ms"]["median"] - t, 4)}
    # the yardstick: brute-force k = 2 of the query against the same candidates' rows, re-supplied from the host
    m = BFMatcher(stream=stream)
    cand = np.stack([db.get_descriptors(int(e)) for e in ids])
    d_cand = DeviceBuffer(cand.nbytes).upload(cand)
    d_q8 = DeviceBuffer(top * q.nbytes).upload(np.stack([q] * top))
    d_n8 = DeviceBuffer(top * 4).upload(np.full(top, rows, np.int32))
    d_kidx, d_kdist = DeviceBuffer(top * rows * 2 * 4), DeviceBuffer(top * rows * 2 * 4)
    knn = lambda: m.knn_match_batch_device(d_q8.ptr, d_n8.ptr, rows, d_cand.ptr, d_n8.ptr, rows, top, 2, d_kidx.ptr, d_kdist.ptr)   # noqa: E731
    res["knn2_resident_ms"] = timed(knn)

    def knn_resupplied():
        check(lib().dvs_memcpy_h2d(0, d_cand.ptr, cand.ctypes.data, cand.nbytes))
        knn()
    res["knn2_with_upload_wall_ms"] = timed(knn_resupplied)         # the copy blocks the host: time between the events, not device time
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
