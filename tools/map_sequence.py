#!/usr/bin/env python3
"""Drives tracker -> mapping backend (dvs_tracker_track -> dvs_backend_add_keyframe_cdr) over the synthetic trajectory, and times
dvs_backend_add_keyframe against the path it replaces.

--track N     N frames of synth.make_traj_frame through the tracker; every keyframe payload goes to the backend with three fixed
              detections; prints the result record per keyframe and the map's size.
--time        per map size (--maps) and keyframe size (--obs): a map of M landmarks with four views each is built through the handle, then
              the same `--keyframes` keyframes of n observations (a new pose, three detections, one class filtered) go
                handle : MappingBackend.add_keyframe — the ctypes call: uploads of the keyframe, all kernels, read-backs, the host walk,
                         the appends.  The map grows by each keyframe's new landmarks while it is timed.
                parent : a host-side database (numpy arrays read back from the handle once, outside the timing) feeding, per class present,
                         FrontendGlue.triangulate_landmarks + FrontendGlue.associate — the entry points the parent commit offers — including
                         the categorisation in numpy, the per-class array rebuild (descriptors, positions, views CSR) and the uploads those
                         calls make.  NOT included: the re-evaluation walk of associateSequential (Python has no binding of
                         dvs_associate_candidates) and the database update, so the figure is a lower bound of that path; its Python and
                         numpy time IS included and was not separated.
              Wall milliseconds per keyframe, median over the keyframes after one warm-up keyframe.  --out writes the JSON."""
import argparse
import json
import os
import sys
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dynamic-visual-slam_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

FX = FY = 500.0; CX, CY = 320.0, 240.0
Q = (0.0, 0.0, 1.0, 0.0)     # R = diag(-1, -1, 1): triangulate's and reprojectPoint's readings of (R, t) agree for t in the x-y plane
DET = [(120.0, 240.0, 90.0, 200.0, "person"), (400.0, 200.0, 220.0, 180.0, "chair"), (450.0, 260.0, 200.0, 200.0, "table")]


def view(X, D, idx, k, rng, noise=0.3):
    t = np.array([0.22 * k, 0.04 * k, 0.0])
    x = X[idx]
    px = np.stack([FX * (-x[:, 0] + t[0]) / x[:, 2] + CX, FY * (-x[:, 1] + t[1]) / x[:, 2] + CY], 1) + rng.normal(0, noise, (len(idx), 2))
    return dict(frame_id=k, stamp=(3 * k, 0), t=t, q=Q, xyz=x + rng.normal(0, 0.03, x.shape), px=px, desc=D[idx])


def add(mb, kf):
    return mb.add_keyframe(kf["frame_id"], kf["stamp"], kf["t"], kf["q"], kf["xyz"], kf["px"], kf["desc"], DET)


def parent_path(glue, db, kf, ids):
    """the categorisation, the per-class rebuild and the two entry points; returns the number of snapshot associations"""
    px = kf["px"].astype(np.float32); x = px[:, 0].astype(np.float64); y = px[:, 1].astype(np.float64)
    cls = np.zeros(len(px), np.int32); free = np.ones(len(px), bool)
    for cx, cy, w, h, name in DET:
        inside = free & (x >= cx - w / 2) & (x <= cx + w / 2) & (y >= cy - h / 2) & (y <= cy + h / 2)
        cls[inside] = ids[name]; free &= ~inside
    R = np.array([-1.0, 0, 0, 0, -1.0, 0, 0, 0, 1.0])
    hits = 0
    for c in np.unique(cls):
        if c == ids["person"]:
            continue
        rows = np.nonzero(db["lm_class"] == c)[0]
        if len(rows) == 0:
            continue
        sel = cls == c
        slot = np.full(len(db["lm_class"]), -1, np.int64); slot[rows] = np.arange(len(rows))
        vs = slot[db["ob_lm_row"]]; keep = np.nonzero(vs >= 0)[0]
        order = keep[np.argsort(vs[keep], kind="stable")]
        offs = np.zeros(len(rows) + 1, np.int64); np.cumsum(np.bincount(vs[keep], minlength=len(rows)), out=offs[1:])
        xyz, _st = glue.triangulate_landmarks(db["kf_R"], db["kf_t"], FX, FY, CX, CY, offs, db["ob_kf"][order], db["ob_px"][order], db["lm_xyz"][rows])
        best = glue.associate(kf["desc"][sel], px[sel], db["lm_desc"][rows], db["lm_xyz"][rows], R, kf["t"], FX, FY, CX, CY)
        hits += int((best >= 0).sum())
    return hits


def time_config(M, n, nkf, seed=3):
    from dvslam_amd import FrontendGlue
    from dvslam_amd.backend import MappingBackend
    rng = np.random.default_rng(seed)
    X = np.stack([rng.uniform(-3.0, 4.0, M), rng.uniform(-2.0, 2.5, M), rng.uniform(2.2, 4.5, M)], 1)
    D = rng.integers(0, 256, (M, 32), dtype=np.uint8)
    mb = MappingBackend(FX, FY, CX, CY, filtered=("person",))
    ids = {name: mb.intern(name) for name in ("person", "chair", "table")}
    for k in range(4):
        add(mb, view(X, D, np.arange(M), k, rng))
    lm, ob, kfs = mb.landmarks(), mb.observations(), mb.keyframes()
    row_of = {int(i): r for r, i in enumerate(lm["id"])}
    kf_of = {int(f): r for r, f in enumerate(kfs["frame_id"])}
    db = dict(lm_class=lm["class_id"], lm_desc=lm["desc"], lm_xyz=lm["xyz"], ob_lm_row=np.array([row_of[int(i)] for i in ob["landmark_id"]], np.int64),
              ob_kf=np.array([kf_of[int(f)] for f in ob["frame_id"]], np.int32), ob_px=ob["px"], kf_R=kfs["R"], kf_t=kfs["t"])
    glue = FrontendGlue()
    tests = [view(X, D, rng.choice(M, n, replace=False), 4 + k, rng) for k in range(nkf + 1)]
    t_handle, t_parent, assoc = [], [], []
    for k, kf in enumerate(tests):
        t0 = time.perf_counter(); hits = parent_path(glue, db, kf, ids); t1 = time.perf_counter()
        r = add(mb, kf); t2 = time.perf_counter()
        if k:                                              # keyframe 0 warms both paths up
            t_parent.append(1e3 * (t1 - t0)); t_handle.append(1e3 * (t2 - t1)); assoc.append((r["n_associated"], hits))
    c = mb.counts()
    mb.close(); glue.close()
    return dict(map_landmarks_at_start=int(len(lm["id"])), map_observations_at_start=int(len(ob["id"])), map_landmarks_at_end=c["n_landmarks"],
                observations_per_keyframe=n, keyframes_timed=nkf, handle_ms_per_keyframe=float(np.median(t_handle)), parent_path_ms_per_keyframe=float(np.median(t_parent)),
                ratio_parent_over_handle=float(np.median(t_parent) / np.median(t_handle)), associated_handle_vs_parent_snapshot=assoc[-1],
                all_runs=dict(handle=t_handle, parent=t_parent))


def track(nframes, cols=640, rows=480, f=600.0, z0=1.5):
    import replay_tracking as rt
    from dvslam_amd import synth, tracker as T
    from dvslam_amd.backend import MappingBackend
    tr = T.Tracker(T.default_params(rows, cols, f, f, cols / 2.0, rows / 2.0))
    mb = MappingBackend(f, f, cols / 2.0, rows / 2.0, filtered=("person",))
    depth = rt.make_depth(rows, cols, z0)
    times = []
    for t in range(nframes):
        r, payload = tr.track(synth.make_traj_frame(t, cols, rows), depth, (t, 0))
        if payload is not None:
            t0 = time.perf_counter(); b = mb.add_keyframe_cdr(payload, DET); times.append(1e3 * (time.perf_counter() - t0))
            print(f"frame {t}: keyframe {r['keyframe_id']} {b} {times[-1]:.3f} ms")
    print("map:", mb.counts())
    tr.close(); mb.close()
    return times


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--track", type=int, default=0)
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--maps", type=int, nargs="+", default=[2000, 20000])
    ap.add_argument("--obs", type=int, nargs="+", default=[200, 1000])
    ap.add_argument("--keyframes", type=int, default=10)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.track:
        track(a.track)
    if a.time:
        out = dict(what="wall milliseconds per keyframe, median: MappingBackend.add_keyframe (handle) against a host-side numpy database feeding "
                        "triangulate_landmarks + associate per class (parent path: rebuild, uploads and Python included; sequential re-evaluation and "
                        "database update not included)", configs=[time_config(M, n, a.keyframes) for M in a.maps for n in a.obs])
        print(json.dumps(out))
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                json.dump(out, fh, indent=1)
