"""The motion-segmentation rule of include/dvslam_hip.h (dvs_motion_*) restated in numpy, operation for operation, plus the scenes and
label patterns the motion tests share.  Not a test module.

The rule.  Inputs: D_ref, D_cur uint16 depth in millimetres; K4 = (fx, fy, cx, cy); R (3 x 3), t (3) with X_ref = R X_cur + t.
  seeds       per current pixel (u, v), float64, every expression left to right as written (numpy evaluates a * b / c as (a * b) / c and
              a + b + c as (a + b) + c, and never fuses):
                valid(d) := min_depth_mm < d <= max_depth_mm (integers); D_cur[v][u] invalid: no verdict
                z = d * 0.001, x = (u - cx) * z / fx, y = (v - cy) * z / fy
                xr = R[0]*x + R[1]*y + R[2]*z + t[0], yr, zr likewise; zr <= 0: no verdict
                ur = floor(fx * xr / zr + cx + 0.5), vr alike; 1 <= ur <= cols - 2 and 1 <= vr <= rows - 2 (as doubles), else no verdict
                all nine D_ref values around (ur, vr) valid, m = their minimum, else no verdict          (n_valid counts who gets here)
                tau = tau0_m + tau2_per_m * zr * zr;  seed iff zr < m * 0.001 - tau
  components  8-connectivity; label = smallest linear index of the component, -1 off the seeds; dynamic iff area >= min_area
  mask        0 iff a dynamic pixel lies in the (2r+1)^2 square around the pixel (outside the image: not dynamic), else 255
Labels come from scipy.ndimage.label (3 x 3 structure) re-labelled to minimum indices, and from a second, plain-Python union-find
(labels_union_find); the dilation from scipy.ndimage.maximum_filter."""
import numpy as np
from scipy import ndimage

DEFAULTS = dict(min_depth_mm=300, max_depth_mm=3000, tau0_m=0.03, tau2_per_m=0.005, min_area=200, dilate_radius=8)
TILE = 32   # DVS_MOTION_TILE: the patterns put their edges on the kernels' tile borders


def seeds(D_ref, D_cur, K4, R, t, **kw):
    """-> (seed bool (rows, cols), n_valid, aux) — aux: per-pixel intermediates for the tests' edge assertions"""
    P = dict(DEFAULTS); P.update(kw)
    rows, cols = D_cur.shape
    fx, fy, cx, cy = (np.float64(k) for k in K4)
    R = np.asarray(R, np.float64).reshape(9); t = np.asarray(t, np.float64).reshape(3)
    lo, hi = int(P["min_depth_mm"]), int(P["max_depth_mm"])
    dc = D_cur.astype(np.int64); dr = D_ref.astype(np.int64)
    v, u = np.mgrid[0:rows, 0:cols]
    u = u.astype(np.float64); v = v.astype(np.float64)
    cur_ok = (lo < dc) & (dc <= hi)
    with np.errstate(all="ignore"):
        z = dc.astype(np.float64) * 0.001
        x = (u - cx) * z / fx
        y = (v - cy) * z / fy
        xr = R[0] * x + R[1] * y + R[2] * z + t[0]
        yr = R[3] * x + R[4] * y + R[5] * z + t[1]
        zr = R[6] * x + R[7] * y + R[8] * z + t[2]
        front = cur_ok & ~(zr <= 0.0)
        ur = np.floor(fx * xr / zr + cx + 0.5)
        vr = np.floor(fy * yr / zr + cy + 0.5)
        inside = front & (1.0 <= ur) & (ur <= float(cols - 2)) & (1.0 <= vr) & (vr <= float(rows - 2))
    iu = np.where(inside, ur, 1).astype(np.int64); iv = np.where(inside, vr, 1).astype(np.int64)
    if rows < 3 or cols < 3:
        inside = np.zeros_like(inside); iu[:] = 0; iv[:] = 0
        win = np.zeros((9, rows, cols), np.int64)
    else:
        win = np.stack([dr[iv + dy, iu + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1)])
    win_ok = (lo < win) & (win <= hi)
    reached = inside & win_ok.all(0)
    m = win.min(0)
    with np.errstate(all="ignore"):
        tau = P["tau0_m"] + P["tau2_per_m"] * zr * zr
        bound = m.astype(np.float64) * 0.001 - tau
        seed = reached & (zr < bound)
    aux = dict(cur_ok=cur_ok, zr=zr, front=front, ur=ur, vr=vr, inside=inside, iu=iu, iv=iv, n_win_invalid=(~win_ok).sum(0), reached=reached,
               m=m, tau=tau, margin=bound - zr)
    return seed, int(reached.sum()), aux


def relabel_min(lab, n):
    """scipy labels 1..n -> the smallest linear index of each component, -1 for 0"""
    flat = lab.ravel()
    out = np.full(flat.shape, -1, np.int32)
    if n:
        first = np.full(n + 1, flat.size, np.int64)
        np.minimum.at(first, flat, np.arange(flat.size))
        out = np.where(flat > 0, first[flat], -1).astype(np.int32)
    return out.reshape(lab.shape)


def labels_scipy(img):
    lab, n = ndimage.label(np.asarray(img) != 0, structure=np.ones((3, 3), int))
    return relabel_min(lab, n)


def labels_union_find(img):
    """the same labels by a plain union-find with path halving, links towards the smaller index"""
    img = np.asarray(img) != 0
    rows, cols = img.shape
    parent = list(range(rows * cols))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    def unite(a, b):
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)
    flat = img.ravel().tolist()
    for yy in range(rows):
        for xx in range(cols):
            p = yy * cols + xx
            if not flat[p]:
                continue
            if xx > 0 and flat[p - 1]:
                unite(p, p - 1)
            if yy > 0:
                if xx > 0 and flat[p - cols - 1]:
                    unite(p, p - cols - 1)
                if flat[p - cols]:
                    unite(p, p - cols)
                if xx + 1 < cols and flat[p - cols + 1]:
                    unite(p, p - cols + 1)
    out = [find(p) if flat[p] else -1 for p in range(rows * cols)]
    return np.array(out, np.int32).reshape(rows, cols)


def areas(labels):
    """area image: the pixel count at every component's root, 0 elsewhere"""
    flat = labels.ravel()
    a = np.zeros(flat.size, np.int32)
    np.add.at(a, flat[flat >= 0], 1)
    return a.reshape(labels.shape)


def mask_from_seeds(seed, min_area, r):
    """-> dict(labels, area, dynamic, mask, and the component statistics)"""
    lab = labels_scipy(seed)
    area = areas(lab)
    dyn = (lab >= 0) & (area.ravel()[np.maximum(lab, 0)] >= min_area)
    dil = ndimage.maximum_filter(dyn.astype(np.uint8), size=2 * r + 1, mode="constant", cval=0)
    mask = np.where(dil > 0, 0, 255).astype(np.uint8)
    return dict(labels=lab, area=area, dynamic=dyn, mask=mask, n_components=int((area > 0).sum()), n_components_kept=int((area >= min_area).sum()),
                n_dynamic=int(dyn.sum()), n_masked=int((mask == 0).sum()))


def segment(D_ref, D_cur, K4, R, t, **kw):
    P = dict(DEFAULTS); P.update(kw)
    seed, n_valid, aux = seeds(D_ref, D_cur, K4, R, t, **P)
    out = mask_from_seeds(seed, P["min_area"], P["dilate_radius"])
    out.update(seed=seed, aux=aux)
    out["stats"] = dict(n_valid=n_valid, n_seed=int(seed.sum()), n_components=out["n_components"], n_components_kept=out["n_components_kept"],
                        n_dynamic=out["n_dynamic"], n_masked=out["n_masked"])
    return out


# ------------------------------------------------------------------------------------------------------------------ scene 1
def rot(axis, deg):
    a = np.deg2rad(deg); c, s = np.cos(a), np.sin(a)
    return {"x": np.array([[1, 0, 0], [0, c, -s], [0, s, c]]), "y": np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]),
            "z": np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])}[axis].astype(np.float64)


def scene1_K(cols, rows):
    f = 0.9 * cols
    return (f, f, cols / 2.0 - 0.5, rows / 2.0 - 0.5)


SCENE1_MOTION = (rot("y", 1.5), np.array([0.06, 0.0, 0.04]))   # current camera in the reference's frame: X_ref = R X_cur + t


def scene1_depth(cols, rows, R=None, t=None, box=None):
    """Ray-cast depth image (uint16 mm) of scene 1 from the camera X_world = R X_cam + t (the reference camera is the world frame):
    a plane slanted about the vertical axis, z = 1.6 + 0.25 x, which steps 0.4 m nearer for x > 0.15 (the step's wall is the plane
    x = 0.15 between the two), and optionally a box face: a fronto-parallel rectangle box = (x0, y0, w, h, z) in world metres."""
    R = np.eye(3) if R is None else np.asarray(R, np.float64)
    t = np.zeros(3) if t is None else np.asarray(t, np.float64)
    fx, fy, cx, cy = scene1_K(cols, rows)
    v, u = np.mgrid[0:rows, 0:cols].astype(np.float64)
    dc = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1)
    dw = dc @ R.T
    a, b, xs, hstep = 1.6, 0.25, 0.15, 0.4
    best = np.full(u.shape, np.inf)

    def hit(s, ok):
        nonlocal best
        with np.errstate(all="ignore"):
            ok = ok & np.isfinite(s) & (s > 0) & (s < best)
        best = np.where(ok, s, best)
    with np.errstate(all="ignore"):
        for off, side in ((0.0, -1), (hstep, 1)):   # z = a + b x - off, on x <= xs (far part) / x >= xs (near part)
            s = (a - off + b * t[0] - t[2]) / (dw[..., 2] - b * dw[..., 0])
            px = t[0] + s * dw[..., 0]
            hit(s, (px - xs) * side >= 0)
        s = (xs - t[0]) / dw[..., 0]                 # the wall
        pz = t[2] + s * dw[..., 2]
        hit(s, (pz >= a + b * xs - hstep) & (pz <= a + b * xs))
        if box is not None:
            x0, y0, w, h, zb = box
            s = (zb - t[2]) / dw[..., 2]
            px = t[0] + s * dw[..., 0]; py = t[1] + s * dw[..., 1]
            hit(s, (px >= x0) & (px <= x0 + w) & (py >= y0) & (py <= y0 + h))
    d = np.rint(np.where(np.isfinite(best), best, 0.0) * 1000.0)   # s is the camera-frame z: the ray direction has z = 1
    return np.clip(d, 0, 65535).astype(np.uint16)


def scene1_box_pixels(cols, rows, R, t, box):
    """the pixels of the camera (R, t) whose ray hits the box face first"""
    return scene1_depth(cols, rows, R, t, box) != scene1_depth(cols, rows, R, t, None)


# ------------------------------------------------------------------------------------------------------------------ scene 2
def scene2(n=12, cols=640, rows=480, block=True, seed=1234, block_seed=77):
    """the tracker tests' scene: the canvas plane at 1500 mm along synth.traj_pose, and a 120 x 160 px block at 900 mm that moves 36 px per
    frame, textured from another canvas seed -> (frames, depths, block boxes (x0, y0, w, h) per frame)"""
    from dvslam_amd import synth
    frames, depths, boxes = [], [], []
    tex = synth._canvas(block_seed, 400, 400)[100:260, 100:220]
    for k in range(n):
        img = synth.make_traj_frame(k, cols, rows, seed=seed).copy()
        d = np.full((rows, cols), 1500, np.uint16)
        x0, y0 = 40 + 36 * k, 160
        if block:
            img[y0:y0 + 160, x0:x0 + 120] = tex
            d[y0:y0 + 160, x0:x0 + 120] = 900
        frames.append(img); depths.append(d); boxes.append((x0, y0, 120, 160))
    return frames, depths, boxes


# ------------------------------------------------------------------------------------------------------------------ label patterns
def spiral(rows, cols):
    g = np.zeros((rows, cols), np.uint8)
    y = x = 0; dy, dx = 0, 1
    g[0, 0] = 1
    while True:
        moved = False
        for _ in range(2):
            ny, nx, my, mx = y + dy, x + dx, y + 2 * dy, x + 2 * dx
            if 0 <= ny < rows and 0 <= nx < cols and not g[ny, nx] and not (0 <= my < rows and 0 <= mx < cols and g[my, mx]):
                y, x = ny, nx; g[y, x] = 1; moved = True
                break
            dy, dx = dx, -dy
        if not moved:
            return g


def patterns(rows, cols):
    """[(name, uint8 image)]: what the labelling must get right — long chains, joins in the last row, tile corners, every tile"""
    yy, xx = np.mgrid[0:rows, 0:cols]
    out = [("empty", np.zeros((rows, cols), np.uint8)), ("full", np.ones((rows, cols), np.uint8)),
           ("checkerboard", ((xx + yy) & 1 == 0).astype(np.uint8)), ("antidiagonals", ((xx + yy) % 3 == 0).astype(np.uint8)),
           ("spiral", spiral(rows, cols))]
    comb = ((xx & 1) == 0).astype(np.uint8); comb[rows - 1, :] = 1
    out.append(("comb", comb))
    corner = np.zeros((rows, cols), np.uint8)   # two 4 x 4 blobs that meet only diagonally, at the corner of four tiles where there is one
    cy, cx = (TILE if rows > TILE else rows // 2), (TILE if cols > TILE else cols // 2)
    corner[max(cy - 4, 0):cy, max(cx - 4, 0):cx] = 1; corner[cy:cy + 4, cx:cx + 4] = 1
    out.append(("diagonal_corner", corner))
    ry, rx = min(TILE // 2, rows - 1), min(TILE // 2, cols - 1)   # a grid of lines, one row and one column through every tile: one component
    out.append(("every_tile", ((yy % TILE == ry) | (xx % TILE == rx)).astype(np.uint8)))
    for dens in (0.3, 0.5, 0.6):
        rng = np.random.default_rng(int(dens * 10) + 1000 * rows + cols)
        out.append((f"random{dens}", (rng.random((rows, cols)) < dens).astype(np.uint8)))
    return out


LABEL_SIZES = [(1, 1), (1, 200), (200, 1), (65, 63), (70, 130)]   # (rows, cols): 1 x 1, 1 x 200, 200 x 1, 63 x 65, 130 x 70 as cols x rows
