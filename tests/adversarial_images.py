"""Deterministic hard inputs for the ORB parity tests (test helper; synth.make_frame stays the benchmark's content).

synth frames are smooth, noisy and mid-grey: FAST candidates are sparse, scores almost never tie and pixels stay away from 0 / 255.
The generators below aim at what those frames never reach: dense candidates on every level (the quad-tree's HBM point path), cells
whose corners have no strict 3x3 maximum (the minThFAST fallback of a cell that is NOT free of corners), tied responses, exact-zero
intensity moments, saturated 0 / 255 content (the signed-byte and packed-f16 range tricks of the kernels) and structures placed on
the cell grid.  Every generator takes (rows, cols), is seeded, and returns a C-contiguous uint8 image.

cell_fast_candidates() restates the per-cell FAST loop of ComputeKeyPointsOctTree (ORBextractor.cpp:781-872) in vectorised numpy,
independently of the oracle's early-exit transcription: the tests use it to bracket the oracle and to assert their preconditions."""
import numpy as np
from dvslam_amd import synth

EDGE_THRESHOLD = 19
RING = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2),
        (-1, 3)]


def iid_noise(rows, cols, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (rows, cols), dtype=np.uint8)


def binary_noise(rows, cols, seed=0):
    return (np.random.default_rng(seed + 1).integers(0, 2, (rows, cols), dtype=np.uint8) * 255).astype(np.uint8)


def checkerboard(rows, cols, period):
    """period x period squares of 0 / 255"""
    yy, xx = np.mgrid[0:rows, 0:cols]
    return np.ascontiguousarray((((yy // period) + (xx // period)) & 1).astype(np.uint8) * 255)


def stripes(rows, cols, period, axis):
    """0 / 255 bars, half a period each (a period-odd bar is one pixel wider dark): aliases under every pyramid resize"""
    idx = np.arange(cols if axis == 1 else rows)
    line = np.where(idx % period < (period + 1) // 2, 0, 255).astype(np.uint8)
    img = np.broadcast_to(line[None, :], (rows, cols)) if axis == 1 else np.broadcast_to(line[:, None], (rows, cols))
    return np.ascontiguousarray(img)


def posterised(rows, cols, t=0, levels=4):
    """the synth frame without sensor noise, quantised to `levels` grey values: plateaus, tied FAST scores, zero IC moments"""
    img = synth.make_frame(t, cols=cols, rows=rows, noise=0).astype(np.int32)
    step = 256 // levels
    return np.ascontiguousarray(np.minimum(img // step, levels - 1) * (255 // (levels - 1))).astype(np.uint8)


def cell_grid(rows, cols, level=0, scale_factor=1.2):
    """(level width, level height, minBorder, wCell, hCell, nCols, nRows) as ComputeKeyPointsOctTree derives them (placement only:
    the level size comes from a float32 power, not the extractor's running product of scale factors)"""
    s = np.float32(1.0) / np.float32(scale_factor) ** level if level else np.float32(1.0)
    w = int(np.rint(np.float32(cols) * s)); h = int(np.rint(np.float32(rows) * s))
    mb = EDGE_THRESHOLD - 3
    width = np.float32(w - EDGE_THRESHOLD + 3 - mb); height = np.float32(h - EDGE_THRESHOLD + 3 - mb)
    ncol = int(width / np.float32(35)); nrow = int(height / np.float32(35))
    return w, h, mb, int(np.ceil(width / np.float32(ncol))), int(np.ceil(height / np.float32(nrow))), ncol, nrow


def boundary_lattice(rows, cols, level=0, scale_factor=1.2):
    """isolated 255-on-0 impulses and 2x2 / 3x3 squares on the cell boundaries iniX + k wCell, iniY + k hCell of `level` (mapped back
    to level-0 pixels) and at +-1..3 px around them: the 6-px cell overlap, the 3-px detection inset of the FAST sub-image and the
    4-column groups / row tail of the wavefront FAST"""
    img = np.zeros((rows, cols), np.uint8)
    _, _, mb, wc, hc, ncol, nrow = cell_grid(rows, cols, level, scale_factor)
    up = float(scale_factor) ** level
    xs = [mb + k * wc + d for k in range(ncol + 1) for d in (-3, 0, 3)]
    ys = [mb + k * hc + d for k in range(nrow + 1) for d in (-3, 0, 3)]
    offs = [-3, -2, -1, 0, 1, 2, 3]
    for a, y in enumerate(ys):
        for b, x in enumerate(xs):
            d = offs[(a * 3 + b) % len(offs)]
            size = (a + 2 * b) % 3 + 1                       # 1 = impulse, 2 / 3 = small squares (tied corners)
            X = int(round((x + (d if b % 2 else 0)) * up)); Y = int(round((y + (0 if b % 2 else d)) * up))
            if 0 <= X and X + size <= cols and 0 <= Y and Y + size <= rows:
                img[Y:Y + size, X:X + size] = 255
    return img


def square_grid(rows, cols, side=20, period=48):
    """flat 255 squares on 0: tied corner scores in nearly every cell"""
    yy, xx = np.mgrid[0:rows, 0:cols]
    return np.ascontiguousarray((((yy % period) < side) & ((xx % period) < side)).astype(np.uint8) * 255)


def sparse_cells(rows, cols, seed=0):
    """a flat frame with contrast in a handful of cells only: almost every cell is empty at both thresholds"""
    rng = np.random.default_rng(seed + 7)
    img = np.full((rows, cols), 110, np.uint8)
    for _ in range(6):
        h = int(rng.integers(12, 40)); w = int(rng.integers(12, 40))
        y = int(rng.integers(30, rows - 30 - h)); x = int(rng.integers(30, cols - 30 - w))
        img[y:y + h, x:x + w] = int(rng.choice([0, 30, 200, 255]))
    return img


def saturated_blocks(rows, cols, seed=0):
    """0 / 255 blocks of 7..40 px edge to edge (independent random row and column cuts)"""
    rng = np.random.default_rng(seed + 11)

    def cuts(n):
        c = np.cumsum(rng.integers(7, 41, n // 7 + 2)); return np.searchsorted(c, np.arange(n), side="right")
    by, bx = cuts(rows), cuts(cols)
    val = rng.integers(0, 2, (by.max() + 1, bx.max() + 1), dtype=np.uint8) * 255
    return np.ascontiguousarray(val[by[:, None], bx[None, :]])


GENERATORS = {
    "iid_noise": iid_noise,
    "binary_noise": binary_noise,
    "checker1": lambda r, c: checkerboard(r, c, 1),
    "checker2": lambda r, c: checkerboard(r, c, 2),
    "checker3": lambda r, c: checkerboard(r, c, 3),
    **{f"stripes{p}{'xy'[ax]}": (lambda r, c, p=p, ax=ax: stripes(r, c, p, 1 - ax)) for p in (2, 3, 4, 5) for ax in (0, 1)},
    "posterised": posterised,
    "lattice0": lambda r, c: boundary_lattice(r, c, 0),
    "lattice2": lambda r, c: boundary_lattice(r, c, 2),
    "square_grid": square_grid,
    "sparse_cells": sparse_cells,
    "saturated": saturated_blocks,
}

_CACHE = {}


def make(name, rows, cols):
    key = (name, rows, cols)
    if key not in _CACHE:
        img = GENERATORS[name](rows, cols)
        assert img.dtype == np.uint8 and img.shape == (rows, cols) and img.flags.c_contiguous
        img.setflags(write=False)
        _CACHE[key] = img
    return _CACHE[key]


# ---------------------------------------------- the per-cell FAST loop in numpy ----------------------------------------------
def fast_best(img):
    """per pixel: the largest b such that 9 contiguous ring pixels all differ from the centre by >= b in one direction (0 on the
    3-px border).  A pixel is a FAST-9 corner at threshold t iff best > t, and cv::FAST's score is then best - 1."""
    I = img.astype(np.int16)
    H, W = I.shape
    best = np.zeros((H, W), np.int16)
    if H < 7 or W < 7:
        return best
    c = I[3:H - 3, 3:W - 3]
    d = np.stack([c - I[3 + dy:H - 3 + dy, 3 + dx:W - 3 + dx] for dx, dy in RING])          # (16, H-6, W-6)
    d = np.concatenate([d, d[:8]])                                                          # wrap-around for the 9-arcs

    def arc9(f):                                        # f over d[k .. k + 8] for k = 0..15 by doubling
        m2 = f(d[:-1], d[1:]); m4 = f(m2[:-2], m2[2:]); m8 = f(m4[:-4], m4[4:])
        return f(m8[:16], d[8:24])
    best[3:H - 3, 3:W - 3] = np.maximum(arc9(np.minimum).max(0), (-arc9(np.maximum)).max(0))
    return best


def _cell_fast(best, y0, y1, x0, x1, t):
    """cv::FAST(sub-image [y0, y1) x [x0, x1), t, nonmax=true): detection inset 3 in the SUB-image, strict 3x3 maximum with
    non-corners (and everything outside the inset) as 0, row-major.  -> (corners exist, [(x, y, score)] in sub-image coordinates)"""
    h, w = y1 - y0, x1 - x0
    sc = np.zeros((h + 2, w + 2), np.int16)                        # one zero ring around the sub-image for the neighbour reads
    if h >= 7 and w >= 7:
        b = best[y0 + 3:y1 - 3, x0 + 3:x1 - 3]
        sc[4:h - 2, 4:w - 2] = np.where(b > t, b - 1, 0)
    corner = sc > 0
    if not corner.any():
        return False, []
    ctr = sc[1:-1, 1:-1]
    nb = np.max(np.stack([sc[1 + dy:h + 1 + dy, 1 + dx:w + 1 + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dy or dx]), axis=0)
    ys, xs = np.nonzero(corner[1:-1, 1:-1] & (ctr > nb))
    return True, [(int(x), int(y), int(ctr[y, x])) for y, x in zip(ys, xs)]


def cell_fast_candidates(level_img, ini_th, min_th, stats=None):
    """ComputeKeyPointsOctTree's cell loop (ORBextractor.cpp:781-872) on one pyramid level: the (w + 6) x (h + 6) sub-image of each
    cell, FAST at iniThFAST, FAST at minThFAST only if that left the cell empty, and the candidates in emission order (cell rows,
    cell columns, then row-major) as (x, y, score) relative to minBorder — the oracle's `candidates(l)` layout.
    stats (dict, optional) receives 'tied_cells': cells with corners at iniThFAST but no strict maximum."""
    best = fast_best(level_img)
    H, W = level_img.shape
    mb = EDGE_THRESHOLD - 3
    maxX, maxY = W - EDGE_THRESHOLD + 3, H - EDGE_THRESHOLD + 3
    width, height = np.float32(maxX - mb), np.float32(maxY - mb)
    ncol, nrow = int(width / np.float32(35)), int(height / np.float32(35))
    wc, hc = int(np.ceil(width / np.float32(ncol))), int(np.ceil(height / np.float32(nrow)))
    out, tied = [], 0
    for i in range(nrow):
        iy = mb + i * hc
        if iy >= maxY - 3:
            continue
        y1 = min(iy + hc + 6, maxY)
        for j in range(ncol):
            ix = mb + j * wc
            if ix >= maxX - 6:
                continue
            x1 = min(ix + wc + 6, maxX)
            any_corner, pts = _cell_fast(best, iy, y1, ix, x1, ini_th)
            if not pts:
                tied += any_corner
                _, pts = _cell_fast(best, iy, y1, ix, x1, min_th)
            out += [(x + j * wc, y + i * hc, s) for x, y, s in pts]
    if stats is not None:
        stats["tied_cells"] = stats.get("tied_cells", 0) + tied
    return np.array(out, np.int32).reshape(-1, 3)
