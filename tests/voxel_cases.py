"""Seeded, directed point clouds for the voxelizer (csrc/voxelize.hip, host twin csrc/voxelize_host.hip), shared by
tests/test_voxel_cases_host.py (which asserts ON THE REFERENCE ALONE that every cloud contains what it was built for, and
that the C oracle, its numpy twin and the library's host entry agree on it bit for bit) and by tests/test_gpu_voxelize.py.

Why directed clouds.  A uniform random point almost never lands within an ulp of a voxel face, so random clouds cannot
tell the float32 add / IEEE divide / floor of utils.py:37-61 from a reciprocal-multiply, an fma-contracted or a float64
chain; they put a handful of voxels over 64 points at most, never n = 63/64/65; and at the two production grids the
ordered compaction (2048-cell tiles, 8 cells per thread, a 256-wide loop over the tile sums) never sees a grid of one
tile, a full grid or a voxel placed on a seam.

Every builder returns (points float32 (N,4), target, overrides); `overrides` is a dict of T/D/H/W that both
oracle.voxelize.grid_for and voxelnet_amd.config.grid_config accept."""
import functools
from collections import namedtuple

import numpy as np

from oracle import voxelize as ov

Case = namedtuple("Case", "id points target overrides")

SCAN_TILE = 2048                          # cells of one tile of k_scan_reduce / k_scan_write (256 threads x 8 cells)
SCAN_WIDTH = 256                          # tile sums per trip of k_scan_blocks
ULPS = 2                                  # neighbours of every voxel face, on both sides
AXES = {"x": ("W", "vx", "ox", 0), "y": ("H", "vy", "oy", 1), "z": ("D", "vz", "oz", 2)}
SEGMENT_T = (1, 35, 45, 64)
SEGMENT_N = (63, 64, 65, 127, 128, 129, 700)            # besides 1, 2, T-1, T, T+1
SMALL_GRIDS = ((1, 3, 5), (1, 32, 64), (1, 1, 2049), (2, 5, 7))       # < one tile, one tile, one tile + 1 cell, odd
COUNTS = (1, 255, 256, 257)               # points of k_key / k_fill: one thread, a workgroup -1 / exact / +1
SLOT_N = 3000


# ------------------------------------------------------------------------------------------------- geometry helpers
def grid(target, overrides):
    return ov.grid_for(target, **overrides)


def axis_centre(g, axis, idx):
    """float32 coordinate of the centre of cell `idx` along `axis`"""
    _, v, o, _ = AXES[axis]
    return ((np.asarray(idx, np.float64) + 0.5) * float(np.float32(g[v])) - float(g[o])).astype(np.float32)


def cell_centres(g, lin):
    """(len(lin), 3) float32 x, y, z of the centres of the linear cells `lin` (z-major, then y, then x: np.unique's order)"""
    lin = np.asarray(lin, np.int64)
    z, y, x = lin // (g["H"] * g["W"]), (lin // g["W"]) % g["H"], lin % g["W"]
    return np.stack([axis_centre(g, "x", x), axis_centre(g, "y", y), axis_centre(g, "z", z)], 1)


def axis_index(points, g, axis, how="ref"):
    """floored voxel index of every point along one axis, as a float array:
    ref    float32 add, float32 IEEE divide (numpy's own; utils.py:37-61)
    recip  float32 add, multiply by the float32 reciprocal of the voxel size
    f64    add, divide and floor in float64 from the float32 inputs (the index is rounded only at the end)"""
    _, v, o, col = AXES[axis]
    x, off, vs = points[:, col].astype(np.float32), np.float32(g[o]), np.float32(g[v])
    with np.errstate(all="ignore"):
        if how == "ref":
            q = (x + off) / vs
        elif how == "recip":
            q = (x + off) * (np.float32(1) / vs)
        elif how == "f64":
            q = (x.astype(np.float64) + np.float64(off)) / np.float64(vs)
        else:
            raise ValueError(how)
        return np.floor(q)


def linear_key(points, g):
    """the reference's linear cell of every point, -1 outside the grid (float32 numpy expressions)"""
    idx = [axis_index(points, g, a) for a in "zyx"]
    ok = np.ones(len(points), bool)
    for f, n in zip(idx, (g["D"], g["H"], g["W"])):
        ok &= (f >= 0) & (f < n)
    z, y, x = (np.where(ok, f, 0).astype(np.int64) for f in idx)
    return np.where(ok, (z * g["H"] + y) * g["W"] + x, -1)


def _intensity(rng, n):
    return rng.uniform(0.0, 1.0, n).astype(np.float32)


def _inside(g, rng, lin, per_cell):
    """`per_cell[i]` distinct points inside cell lin[i], away from its faces; rows grouped by cell"""
    lin = np.repeat(np.asarray(lin, np.int64), per_cell)
    c = cell_centres(g, lin).astype(np.float64)
    half = 0.45 * np.array([g["vx"], g["vy"], g["vz"]])
    xyz = (c + rng.uniform(-1.0, 1.0, c.shape) * half).astype(np.float32)
    return np.concatenate([xyz, _intensity(rng, len(lin))[:, None]], 1), lin


# ------------------------------------------------------------------------------------------------- boundary cloud
def boundary_axis_points(target, axis):
    """the points of boundary_cloud(target) that probe the faces of one axis, before the shuffle: for every face
    k = 0..n, float32(k * v - o) and its neighbours at -2..+2 ulp; the other two coordinates sit at a cell centre that
    changes from point to point"""
    g = grid(target, {})
    n, v, o, col = AXES[axis]
    rng = np.random.default_rng(1000 + 10 * (target == "Car") + col)
    face = (np.arange(g[n] + 1, dtype=np.float64) * float(np.float32(g[v])) - float(g[o])).astype(np.float32)
    cols = [face]
    for sign in (-np.inf, np.inf):
        f = face
        for _ in range(ULPS):
            f = np.nextafter(f, np.float32(sign))
            cols.append(f)
    probe = np.stack(cols, 1).reshape(-1)                        # (n+1) * (2*ULPS+1)
    j = np.arange(probe.size)
    pts = np.empty((probe.size, 4), np.float32)
    others = [a for a in "xyz" if a != axis]
    for a, mul, add in zip(others, (7, 3), (3, 1)):
        pts[:, AXES[a][3]] = axis_centre(g, a, (j * mul + add) % g[AXES[a][0]])
    pts[:, col] = probe
    pts[:, 3] = _intensity(rng, probe.size)
    return pts


@functools.lru_cache(maxsize=None)
def _boundary(target):
    pts = np.concatenate([boundary_axis_points(target, a) for a in "xyz"])
    np.random.default_rng(7 + (target == "Car")).shuffle(pts)
    pts.setflags(write=False)
    return pts


def boundary_cloud(target):
    return _boundary(target), target, {}


# ------------------------------------------------------------------------------------------------ non-finite cloud
@functools.lru_cache(maxsize=None)
def nonfinite_parts():
    """name -> (n,4) float32 rows of nonfinite_cloud(), Car grid.  Every special row has an intensity of its own, so a
    row can be found again in a feature buffer by its bits."""
    g = grid("Car", {})
    rng = np.random.default_rng(21)
    parts = {}
    base, _ = _inside(g, rng, rng.choice(g["D"] * g["H"] * g["W"], 150, replace=False), 2)
    parts["ordinary"] = base
    tag = iter(np.float32(2.0) + np.arange(200, dtype=np.float32))          # intensities 2, 3, ...: not in [0, 1)

    def row(x=10.1, y=0.1, z=-1.0, w=None):
        return np.array([[x, y, z, next(tag) if w is None else w]], np.float32)

    sub = np.float32(np.nextafter(np.float32(0), np.float32(1)))              # 2^-149
    bad = []
    for val in (np.nan, np.inf, -np.inf, 1e30, -1e30):
        bad += [row(x=val), row(y=val), row(z=val)]
    parts["bad_coordinate"] = np.concatenate(bad)                             # all dropped
    parts["neg_zero_x"] = row(x=-0.0, y=3.3, z=-0.5)                          # -0 + 0 = +0: kept, cell x = 0
    parts["neg_subnormal_x"] = row(x=-sub, y=3.3, z=-0.5)                     # floor(-2^-149 / 0.2) = -1: dropped
    parts["pos_subnormal_x"] = row(x=sub, y=5.5, z=-0.5)                      # kept, cell x = 0
    parts["odd_intensity"] = np.concatenate([row(x=20.1, w=np.nan), row(x=20.1, w=np.inf), row(x=30.1, w=-np.inf),
                                             row(x=30.1, w=np.float32(-0.0))])             # kept, bits carried through
    # two voxels whose kept points have a negative zero in a coordinate: y = -0 (cell y = 200), z = -0 (cell z = 7); the
    # first has nothing but -0 in y, so its centroid is +0 and its offsets are -0 - +0 = -0
    parts["neg_zero_voxels"] = np.concatenate([row(x=40.1, y=-0.0), row(x=40.15, y=-0.0), row(x=40.05, y=-0.0),
                                               row(x=50.1, z=-0.0), row(x=50.15, z=-0.0), row(x=50.05, z=-0.2)])
    for v in parts.values():
        v.setflags(write=False)
    return parts


@functools.lru_cache(maxsize=None)
def _nonfinite():
    pts = np.concatenate(list(nonfinite_parts().values()))
    np.random.default_rng(22).shuffle(pts)
    pts.setflags(write=False)
    return pts


def nonfinite_cloud():
    return _nonfinite(), "Car", {}


# -------------------------------------------------------------------------------------------------- segment cloud
def segment_sizes(T):
    out = []
    for n in (1, 2, T - 1, T, T + 1) + SEGMENT_N:
        if n >= 1 and n not in out:
            out.append(n)
    return out


@functools.lru_cache(maxsize=None)
def _segment(T):
    target = "Pedestrian" if T == 45 else "Car"
    g = grid(target, {"T": T})
    rng = np.random.default_rng(300 + T)
    sizes = segment_sizes(T)
    cells = g["D"] * g["H"] * g["W"]
    hot = rng.choice(cells, len(sizes), replace=False)
    rows = []
    for c, n in zip(hot, sizes):
        dup = 3 if n >= 5 else 0                      # n input points: n - dup distinct ones + dup copies of one of them
        p, _ = _inside(g, rng, [c], [n - dup])
        rows.append(np.concatenate([p, np.repeat(p[rng.integers(n - dup)][None], dup, 0)]))
    free = np.setdiff1d(np.arange(cells), hot)
    bg, _ = _inside(g, rng, rng.choice(free, 300), 1)
    pts = np.concatenate(rows + [bg]).astype(np.float32)
    rng.shuffle(pts)                                  # one permutation over all voxels' points
    pts.setflags(write=False)
    return pts, target


def segment_cloud(T):
    pts, target = _segment(T)
    return pts, target, {"T": T}


# ------------------------------------------------------------------------------------------------ tile-seam cloud
def tile_seam_cells():
    """the distinct linear cells of tile_seam_cloud(), ascending"""
    g = grid("Car", {})
    cells = g["D"] * g["H"] * g["W"]
    single = [0, 7, 8, SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1]
    for t in (SCAN_WIDTH - 1, SCAN_WIDTH, 2 * SCAN_WIDTH):
        single += [SCAN_TILE * t - 1, SCAN_TILE * t + 1]
    single += [cells - 2, cells - 1]
    aligned = np.arange(SCAN_TILE) + SCAN_TILE * 300                      # starts at a tile boundary
    straddle = np.arange(SCAN_TILE) + SCAN_TILE * 400 + 1000              # straddles one
    return np.unique(np.concatenate([single, aligned, straddle]).astype(np.int64))


@functools.lru_cache(maxsize=None)
def _tile_seam():
    g = grid("Car", {})
    lin = tile_seam_cells()
    rng = np.random.default_rng(41)
    per = rng.integers(1, 3, len(lin))                                    # one or two points at each cell
    lin = np.repeat(lin, per)
    pts = np.concatenate([cell_centres(g, lin), _intensity(rng, len(lin))[:, None]], 1).astype(np.float32)
    rng.shuffle(pts)
    pts.setflags(write=False)
    return pts


def tile_seam_cloud():
    return _tile_seam(), "Car", {}


# ---------------------------------------------------------------------------------------------------- small grids
@functools.lru_cache(maxsize=None)
def small_grid_clouds():
    """[(id, points, target, overrides)]: per grid a fully occupied one (1..3 points in every cell: K == cells < N) and
    one point in each of half of the cells (K == N)"""
    out = []
    for D, H, W in SMALL_GRIDS:
        over = {"D": D, "H": H, "W": W}
        g = grid("Car", over)
        cells = D * H * W
        rng = np.random.default_rng(500 + cells)
        per = rng.integers(1, 4, cells)
        per[0] = 3                                                        # N > cells whatever the seed
        full, _ = _inside(g, rng, np.arange(cells), per)
        half, _ = _inside(g, rng, np.sort(rng.choice(cells, (cells + 1) // 2, replace=False)), 1)
        for name, pts in (("full", full), ("half", half)):
            rng.shuffle(pts)
            pts.setflags(write=False)
            out.append(Case(f"grid{D}x{H}x{W}-{name}", pts, "Car", over))
    return out


# --------------------------------------------------------------------------------------------------- point counts
@functools.lru_cache(maxsize=None)
def count_clouds():
    """[(id, points, target, overrides)]: N points in N voxels, and the same N points moved out of range (K = 0)"""
    g = grid("Car", {})
    out = []
    for n in COUNTS:
        rng = np.random.default_rng(600 + n)
        pts, _ = _inside(g, rng, rng.choice(g["D"] * g["H"] * g["W"], n, replace=False), 1)
        rng.shuffle(pts)
        far = pts.copy()
        far[:, 0] += np.float32(100.0)                                    # x >= 70.4
        for name, p in ((f"count{n}", pts), (f"count{n}-outside", far)):
            p.setflags(write=False)
            out.append(Case(name, p, "Car", {}))
    return out


# ------------------------------------------------------------------------------------------------------ slot reuse
@functools.lru_cache(maxsize=None)
def slot_reuse_clouds():
    """three Car clouds of the same N for one VoxelBuffers slot, in the order they go through it: large K, small K, K = 0"""
    g = grid("Car", {})
    rng = np.random.default_rng(77)
    cells = g["D"] * g["H"] * g["W"]
    large, _ = _inside(g, rng, rng.choice(cells, SLOT_N - 200, replace=False), 1)
    more, _ = _inside(g, rng, rng.choice(cells, 20, replace=False), 10)
    large = np.concatenate([large, more])
    small, _ = _inside(g, rng, rng.choice(cells, 6, replace=False), SLOT_N // 6)
    none = large.copy()
    none[:, 1] -= np.float32(200.0)                                       # y < -40
    out = []
    for name, p in (("slot-large", large), ("slot-small", small), ("slot-none", none)):
        rng.shuffle(p)
        assert p.shape == (SLOT_N, 4)
        p.setflags(write=False)
        out.append(Case(name, p, "Car", {}))
    return out


# ------------------------------------------------------------------------------------------------------- registry
@functools.lru_cache(maxsize=None)
def all_cases():
    out = [Case(f"boundary-{t}", *boundary_cloud(t)) for t in ("Car", "Pedestrian")]
    out.append(Case("nonfinite", *nonfinite_cloud()))
    out += [Case(f"segment-T{T}", *segment_cloud(T)) for T in SEGMENT_T]
    out.append(Case("tile-seam", *tile_seam_cloud()))
    out += small_grid_clouds() + count_clouds() + slot_reuse_clouds()
    return out


def case(case_id):
    return next(c for c in all_cases() if c.id == case_id)


@functools.lru_cache(maxsize=None)
def reference(case_id):
    """the C oracle's buffers for a case: computed once, shared, read-only"""
    c = case(case_id)
    with np.errstate(all="ignore"):
        ref = ov.voxelize(c.points, c.target, **c.overrides)
    for v in ref.values():
        v.setflags(write=False)
    return ref
