"""Run ON THE GPU BOX (under rocprofv3 --kernel-trace --stats for per-kernel times, k_cand_mask among them): dvs_orb_extract_batch_device
on 64 synthetic 1280 x 720 frames at 2000 keypoints, unmasked and with per-frame box masks that zero about 30 % of the pixels,
interleaved call by call on one handle.  Each sample is the host wall time of one call plus its synchronisation.  Prints one JSON
line: median / min milliseconds of each form and the masked overhead."""
import json
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dynamic-visual-slam_amd"))
import torch  # noqa: E402,F401  (first: one ROCm runtime for the process, see tests/conftest.py)
import numpy as np  # noqa: E402
import dvslam_amd  # noqa: E402
from dvslam_amd import _lib, synth  # noqa: E402

B, ROWS, COLS, NF = 64, 720, 1280, 2000
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
imgs = np.stack([synth.make_frame(t, cols=COLS, rows=ROWS) for t in range(B)])
masks = np.full((B, ROWS, COLS), 255, np.uint8)
for f in range(B):   # three boxes per frame, moving with f: 0.30 of the frame
    for (x, y, w, h) in ((100, 150, 300, 400), (600, 100, 260, 420), (950, 250, 220, 240)):
        masks[f, y:y + h, x + 2 * f:x + 2 * f + w] = 0
covered = float((masks == 0).mean())
g = dvslam_amd.ORBextractor(NF, 1.2, 8, 20, 7, max_batch=B)
cap = g.capacity
d_img = _lib.DeviceBuffer(imgs.nbytes).upload(imgs)
d_mask = _lib.DeviceBuffer(masks.nbytes).upload(masks)
d_k = _lib.DeviceBuffer(B * cap * 28); d_d = _lib.DeviceBuffer(B * cap * 32); d_n = _lib.DeviceBuffer(4 * B)


def call(masked):
    g.extract_batch_device(d_img.ptr, B, ROWS, COLS, COLS, ROWS * COLS, d_k.ptr, d_d.ptr, cap, d_n.ptr,
                           d_masks=d_mask.ptr if masked else None)


for _ in range(5):
    call(False); call(True)
g.synchronize()
t = {False: [], True: []}
for r in range(reps):
    for masked in ((False, True) if r % 2 == 0 else (True, False)):
        t0 = time.perf_counter()
        call(masked)
        g.synchronize()
        t[masked].append(1e3 * (time.perf_counter() - t0))
n_masked = d_n.download(np.int32, B)
call(False); g.synchronize()
n_plain = d_n.download(np.int32, B)
res = {"frames": B, "mask_zero_fraction": round(covered, 3),
       "unmasked_ms_median": round(float(np.median(t[False])), 4), "masked_ms_median": round(float(np.median(t[True])), 4),
       "unmasked_ms_min": round(float(np.min(t[False])), 4), "masked_ms_min": round(float(np.min(t[True])), 4),
       "keypoints_per_frame_unmasked": float(n_plain.mean()), "keypoints_per_frame_masked": float(n_masked.mean())}
res["masked_over_unmasked"] = round(res["masked_ms_median"] / res["unmasked_ms_median"], 4)
print(json.dumps(res))
