"""Run ON THE GPU BOX (under rocprofv3 --kernel-trace --stats for per-kernel times): the matcher modes on 64 jobs of 2000 x 2000 synthetic
descriptors (the streaming step's match shape), timed with device events and interleaved with the plain arg-min match in the same
process: match, knn k = 2 / 4 / 8, crossCheck, radius at 100.  Prints one JSON line: median microseconds per call of each."""
import json
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dynamic-visual-slam_amd"))
import torch  # noqa: E402  (first: one ROCm runtime for the process, see tests/conftest.py)
import numpy as np  # noqa: E402
import dvslam_amd  # noqa: E402
from dvslam_amd import _lib, synth  # noqa: E402

P, S, N = 64, 2048, 2000
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
stream = torch.cuda.current_stream()
m = dvslam_amd.BFMatcher(stream=stream.cuda_stream)
Q = np.stack([synth.make_descriptors(S, 1000 + p) for p in range(P)]); T = np.stack([synth.make_descriptors(S, 2000 + p) for p in range(P)])
n = np.full(P, N, np.int32)
dq = _lib.DeviceBuffer(Q.nbytes).upload(Q); dt = _lib.DeviceBuffer(T.nbytes).upload(T); dn = _lib.DeviceBuffer(n.nbytes).upload(n)
di = _lib.DeviceBuffer(P * S * 8 * 4); dd = _lib.DeviceBuffer(P * S * 8 * 4)
q1 = np.ascontiguousarray(Q[0, :N]); t1 = np.ascontiguousarray(T[0, :N])

calls = {
    "match": lambda: m.match_batch_device(dq.ptr, dn.ptr, S, dt.ptr, dn.ptr, S, P, di.ptr, dd.ptr),
    "knn2": lambda: m.knn_match_batch_device(dq.ptr, dn.ptr, S, dt.ptr, dn.ptr, S, P, 2, di.ptr, dd.ptr),
    "knn4": lambda: m.knn_match_batch_device(dq.ptr, dn.ptr, S, dt.ptr, dn.ptr, S, P, 4, di.ptr, dd.ptr),
    "knn8": lambda: m.knn_match_batch_device(dq.ptr, dn.ptr, S, dt.ptr, dn.ptr, S, P, 8, di.ptr, dd.ptr),
    "cross": lambda: m.cross_match_batch_device(dq.ptr, dn.ptr, S, dt.ptr, dn.ptr, S, P, di.ptr, dd.ptr),
}
times = {k: [] for k in calls}
for _ in range(3):
    for f in calls.values():
        f()
torch.cuda.synchronize()
for r in range(reps):
    for name, f in calls.items():   # interleaved: every mode sits beside a plain match in time
        a = torch.cuda.Event(enable_timing=True); b = torch.cuda.Event(enable_timing=True)
        a.record(stream); f(); b.record(stream)
        b.synchronize()
        times[name].append(1e3 * a.elapsed_time(b))
# radius: a host entry point (count, scan, write, sort + copies), one 2000 x 2000 job per call, 64 calls = the 64 jobs
radius = []
for r in range(max(reps // 10, 3)):
    a = torch.cuda.Event(enable_timing=True); b = torch.cuda.Event(enable_timing=True)
    a.record(stream)
    tot = 0
    for p in range(P):
        offs, idx, dist = m.radius_match(Q[p, :N], T[p, :N], 100.0)
        tot += len(idx)
    b.record(stream); b.synchronize()
    radius.append(1e3 * a.elapsed_time(b))
res = {k: round(float(np.median(v)), 1) for k, v in times.items()}
res["radius100_64jobs_host"] = round(float(np.median(radius)), 1)
res["radius100_pairs"] = tot
res.update({f"{k}_over_match": round(res[k] / res["match"], 2) for k in calls if k != "match"})
print(json.dumps(res))
