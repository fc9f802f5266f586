"""Inputs of the anchor-mask tests: seeded voxel sets, hand-made rectangle tables and hand-made
anchors.  tests/test_anchor_mask_host.py asserts the guards on the reference alone; tests/test_gpu_anchor_mask.py
compares the kernels with tests/anchor_mask_ref.py on exactly these inputs."""
import os
import re

import numpy as np

import anchor_mask_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = open(os.path.join(ROOT, "voxelnet-pytorch_amd", "csrc", "anchor_mask.hip")).read()
ROW_CHUNK = int(re.search(r"constexpr int AM_THREADS = (\d+);", _SRC).group(1))          # cells per trip of the row scan
COL_SEG = int(re.search(r"constexpr int AM_SEG = (\d+);", _SRC).group(1))                  # rows per column segment
D, B = 10, 3
THRESHOLDS = (0, 1, 5)          # (+ one above every count, taken from the reference's counts)

# (H, W): which seam each crosses
GRIDS = {
    (1, 1): "the smallest grid: one cell, one (partial) chunk, one (partial) segment",
    (3, 5): "a grid below every tile",
    (7, ROW_CHUNK): "exactly one row-scan chunk wide: no carry",
    (7, ROW_CHUNK + 1): "a chunk plus one cell: the carry into a second trip of the row scan; the table's W + 1 columns need a second "
                        "workgroup column in the column pass",
    (COL_SEG, 9): "exactly one column segment high: no segment total is read",
    (COL_SEG + 1, 9): "a segment plus one row: the second segment reads the first's total",
    (2 * COL_SEG + 1, 9): "two segments plus one row: a carry summed over two totals",
    (130, 300): "both at once, neither size a multiple of its tile",
}


def voxels(H, W, seed=0):
    """(K, 4) int64 rows [b, d, h, w] of a batch of B = 3 with (many, 0, 1) voxels: the two corners, a full stack of D in
    one cell, every cell of one row and of one column (non-zero carries across every chunk and segment boundary), seeded
    extras, and four rows that must change nothing (b = -1, b = B, h = H, w = -1); shuffled"""
    rng = np.random.default_rng(1000 * H + W + seed)
    rows = [(0, 0, 0, 0), (0, D - 1, H - 1, W - 1)]
    rows += [(0, d, H // 2, W // 2) for d in range(D)]
    rows += [(0, 1, H // 3, w) for w in range(W)]
    rows += [(0, 2, h, (2 * W) // 3) for h in range(H)]
    extra = min(4 * H * W, 3000)
    rows += list(zip([0] * extra, rng.integers(0, D, extra), rng.integers(0, H, extra), rng.integers(0, W, extra)))
    rows += [(2, 3, H - 1, 0)]
    rows += [(-1, 0, 0, 0), (B, 0, 0, 0), (0, 0, H, 0), (0, 0, 0, -1)]
    c = np.array(rows, dtype=np.int64)
    return np.ascontiguousarray(c[rng.permutation(c.shape[0])])


def rect_table(H, W, seed=0):
    """(N, 4) int32 [w0, h0, w1, h1]: single cells, the whole grid, rectangles clipped on each side (components outside the
    grid: the device clips them), the empty rectangle as anchor_cell_rects stores it, other empty ones, rectangles ending
    and starting at every seam and at every seam + 1, seeded ones"""
    t = [(0, 0, 0, 0), (W - 1, H - 1, W - 1, H - 1), (W // 2, H // 2, W // 2, H // 2), (0, 0, W - 1, H - 1),
         (-3, 0, W // 2, H - 1), (W // 2, 0, W + 2, H - 1), (0, -2, W - 1, H // 2), (0, H // 2, W - 1, H + 5), (-9, -9, W + 9, H + 9),
         (0, 0, -1, -1), (3, 0, 2, H - 1), (0, 3, W - 1, 2), (W, 0, W + 4, H - 1), (0, H, W - 1, H + 4), (-5, 0, -1, H - 1)]
    for s in (ROW_CHUNK - 1, ROW_CHUNK, ROW_CHUNK + 1):
        if s < W:
            t += [(0, 0, s, H - 1), (s, 0, W - 1, H - 1), (s, H // 3, s, H // 3)]
    for k in (1, 2):
        for s in (k * COL_SEG - 1, k * COL_SEG, k * COL_SEG + 1):
            if s < H:
                t += [(0, 0, W - 1, s), (0, s, W - 1, H - 1), ((2 * W) // 3, s, (2 * W) // 3, s)]
    rng = np.random.default_rng(77 * H + W + seed)
    for _ in range(40):
        w0, w1 = np.sort(rng.integers(0, W, 2))
        h0, h1 = np.sort(rng.integers(0, H, 2))
        t.append((w0, h0, w1, h1))
    return np.ascontiguousarray(np.array(t, dtype=np.int32))


def tiny_grid():
    """the 10 x 16 x 24 grid of the tiny model fixtures: the Car grid's voxel size and offsets, H = 16, W = 24"""
    from dataclasses import replace
    from voxelnet_amd.config import grid_config
    return replace(grid_config("Car"), H=16, W=24)


def hand_anchors():
    """{name: (anchors (h, w, 2, 7) float64, grid)}: hand-made anchor sets on the tiny grid — edges on cell boundaries, turned
    boxes, boxes over each border, entirely outside, of zero size"""
    g = tiny_grid()
    y0 = -float(g.oy)

    def grid_of(rows):
        a = np.array(rows, dtype=np.float64)
        return a.reshape(-1, 1, 2, 7)
    sets = {
        # l = 0.8, w = 0.4 at multiples of 0.2: every edge of the unturned and of the quarter-turned box is on a boundary
        "on_boundaries": grid_of([[1.0, y0 + 1.0, -1, 1.5, 0.4, 0.8, 0.0], [1.0, y0 + 1.0, -1, 1.5, 0.4, 0.8, np.pi / 2],
                                  [2.4, y0 + 2.0, -1, 1.5, 0.8, 1.6, 0.0], [2.4, y0 + 2.0, -1, 1.5, 0.8, 1.6, np.pi / 2]]),
        "turned": grid_of([[2.13, y0 + 1.57, -1, 1.5, 1.6, 3.9, 0.3], [2.13, y0 + 1.57, -1, 1.5, 1.6, 3.9, -1.1],
                           [3.31, y0 + 0.77, -1, 1.5, 0.6, 1.76, 2.5], [0.93, y0 + 2.21, -1, 1.5, 0.6, 0.8, 0.7]]),
        "borders": grid_of([[0.05, y0 + 1.63, -1, 1.5, 1.6, 3.9, 0.0], [4.71, y0 + 1.63, -1, 1.5, 1.6, 3.9, 0.0],
                            [2.33, y0 + 0.07, -1, 1.5, 1.6, 3.9, np.pi / 2], [2.33, y0 + 3.11, -1, 1.5, 1.6, 3.9, np.pi / 2],
                            [2.33, y0 + 1.63, -1, 1.5, 30.0, 30.0, 0.4], [0.0, y0, -1, 1.5, 0.3, 0.3, 0.0]]),
        "outside_or_empty": grid_of([[-5.03, y0 + 1.0, -1, 1.5, 1.6, 3.9, 0.0], [9.77, y0 + 1.0, -1, 1.5, 1.6, 3.9, 0.0],
                                     [2.0, y0 - 4.13, -1, 1.5, 1.6, 3.9, 0.0], [2.0, y0 + 9.31, -1, 1.5, 1.6, 3.9, 0.0],
                                     [1.0, y0 + 1.0, -1, 1.5, 0.0, 0.0, 0.0], [1.07, y0 + 1.03, -1, 1.5, 0.0, 0.0, 0.0]]),
    }
    return {k: (v, g) for k, v in sets.items()}


def min_unsnapped_gap(anchors, grid):
    """the guard: the smallest distance to an integer of any rectangle edge (in cells) that the snap does NOT move — the
    rule is safe for an anchor set when nothing lies between the snap distance and ordinary values: no component in
    (1e-9, 1e-6) of an integer.  Also returns how many components the snap moves (edges on a cell boundary)."""
    gap = R.boundary_gap(R.rect_q(anchors, grid))
    gap = gap[np.isfinite(gap)]
    on = gap <= R.SNAP
    return (float(gap[~on].min()) if (~on).any() else float("inf")), int(on.sum())


def full_frame(cls_name, B=2, per_frame=20000, seed=5):
    """(K, 4) int64 coordinates of B frames with ~per_frame distinct seeded voxels each on the class's grid: a wedge
    of ground returns that thins with range plus clusters, so that a large share of the anchors has nothing under it"""
    from voxelnet_amd.config import grid_config
    g = grid_config(cls_name)
    rng = np.random.default_rng(seed)
    out = []
    for b in range(B):
        r = np.abs(rng.normal(0.0, 0.35, 3 * per_frame)) * g.W
        th = rng.uniform(-0.7, 0.7, 3 * per_frame)
        w = np.floor(r * np.cos(th)).astype(np.int64)
        h = np.floor(g.H / 2 + r * np.sin(th)).astype(np.int64)
        d = rng.integers(0, g.D, 3 * per_frame)
        ok = (w >= 0) & (w < g.W) & (h >= 0) & (h < g.H)
        cells = np.unique(np.stack([d[ok], h[ok], w[ok]], axis=1), axis=0)
        cells = cells[rng.permutation(cells.shape[0])[:per_frame]]
        out.append(np.concatenate([np.full((cells.shape[0], 1), b, dtype=np.int64), cells], axis=1))
    return np.ascontiguousarray(np.concatenate(out, axis=0)), g
