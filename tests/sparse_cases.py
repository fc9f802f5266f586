"""Directed occupancy sets for the sparse first Conv3d (middle_layer.0: Conv3d 128 -> 64, k 3, stride (2,1,1), pad (1,1,1);
csrc/sparse.hip, the row-list modes of csrc/conv.hip and csrc/wgrad.hip), shared by tests/test_sparse_cases_host.py (which
proves ON THE ORACLE ALONE that every set holds what it was built for) and tests/test_gpu_sparse_first_layer.py.

Why directed sets.  3000 uniformly random cells of a 2 x 10 x 134 x 140 grid (the one kernel-level test of this layer so
far) give almost every active site exactly one contributing voxel and none all 27; they touch a grid corner only by luck;
their ~50 k active sites stay below the 131 072 (RB_MAX_BLOCKS * RB_ROWS) at which k_rulebook_combine takes a second
persistent trip and their 187 600 output sites (92 scan tiles) below the 256 tiles at which the ordered compaction's
single-block scan takes its carry trip; and no list has a length of k * 256 +- 1 or k * 64 +- 1.

The oracle of the active-site list does not restate k_mark's index arithmetic: a site is active iff
conv3d(occupancy, ones(3,3,3), stride, pad) > 0 there, and the list is those sites in ascending linear (b, d, h, w) order.

Every case is (id, B, D, H, W, coord int64 (K,4) [b, z, y, x]); the voxel order is deliberately NOT sorted."""
import functools
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

Case = namedtuple("Case", "id B D H W coord")

KERNEL, STRIDE, PAD = (3, 3, 3), (2, 1, 1), (1, 1, 1)
CIN, COUT = 128, 64
SCAN_TILE = 2048            # output sites per tile of the ordered compaction (256 threads x 8 sites)
SCAN_WIDTH = 256            # tile sums per trip of the single-block scan
LIST_TILE = 256             # list rows per tile of the row-list gather GEMM (BM = 256 at Cout = 64)
RB_ROWS, RB_MAX_BLOCKS = 64, 2048       # k_rulebook_combine: list rows per block, workgroups of its persistent loop
PER_VOXEL = 18              # most active sites one voxel can have: ceil(3/2) * 3 * 3

COUNT_TARGETS = (255, 256, 257, 63, 64, 65)
K_TARGETS = (255, 256, 257)
COUNT_GRID = (1, 10, 15, 33)


def out_dims(D, H, W):
    return tuple((d + 2 * p - k) // s + 1 for d, p, k, s in zip((D, H, W), PAD, KERNEL, STRIDE))


def _shuffled(rows, seed):
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 4)
    return rows[np.random.default_rng(seed).permutation(len(rows))]


def _unravel(cells, D, H, W):
    cells = np.asarray(cells, dtype=np.int64)
    return np.stack([cells // (D * H * W), (cells // (H * W)) % D, (cells // W) % H, cells % W], 1)


def _random_cells(B, D, H, W, K, seed):
    """K distinct cells in a seeded random ORDER (rng.choice without replacement does not sort)"""
    return _unravel(np.random.default_rng(seed).choice(B * D * H * W, size=K, replace=False), D, H, W)


def _full_block():
    B, D, H, W = 2, 5, 6, 7
    return Case("full_block", B, D, H, W, _shuffled(_unravel(np.arange(B * D * H * W), D, H, W), 11))


def _corners_faces():
    B, D, H, W = 2, 4, 6, 7
    rows = []
    for b in range(B):
        rows += [(b, z, y, x) for z in (0, D - 1) for y in (0, H - 1) for x in (0, W - 1)]
        rows += [(b, 0, H // 2, W // 2), (b, D - 1, H // 2, W // 2), (b, D // 2, 0, W // 2), (b, D // 2, H - 1, W // 2),
                 (b, D // 2, H // 2, 0), (b, D // 2, H // 2, W - 1)]
    return Case("corners_faces", B, D, H, W, _shuffled(rows, 12))


def _batch_seam():
    B, D, H, W = 2, 4, 6, 7
    return Case("batch_seam", B, D, H, W, np.array([(1, 0, 0, 0), (0, D - 1, H - 1, W - 1)], dtype=np.int64))


def _one_item_empty():
    return Case("one_item_empty", 2, 4, 6, 7, _shuffled([(1, 0, 2, 3), (1, 2, 4, 1), (1, 3, 5, 6), (1, 1, 0, 0), (1, 2, 4, 2)], 13))


def _single():
    return Case("single", 1, 4, 6, 7, np.array([(0, 1, 3, 3)], dtype=np.int64))


def _empty():
    return Case("empty", 1, 4, 6, 7, np.zeros((0, 4), dtype=np.int64))


def _depth_parity():
    """one voxel at every z = 0..9 of a 10 x 8 x 9 grid.  An 8 x 9 plane holds nine H/W-disjoint 3 x 3 windows (centres
    1, 4, 7 on both axes); z = 0 (output depth 0 only) and z = 9 (output depth 4 only: its upper tap would be depth 5 of
    Do = 5) share one.  The host test proves that no output site sees two voxels."""
    slots = [(y, x) for y in (1, 4, 7) for x in (1, 4, 7)]
    rows = [(0, z) + slots[z % 9] for z in range(10)]
    return Case("depth_parity", 1, 10, 8, 9, _shuffled(rows, 14))


def _count_case(n):
    """isolated voxels of a 1 x 10 x 15 x 33 grid whose active-site count is exactly n = 18 a + 9 b + 6 c + 4 d:
    a interior voxels at odd z < 9 (two output depths x 3 x 3), b interior at even z (one depth), c at even z in the
    middle of the y = 0 / y = H - 1 edge (2 x 3), d at even z in a corner of the plane (2 x 2).  Every voxel but the
    corner ones has an H/W window of its own; the corner ones sit on distinct even z, i.e. distinct output depths."""
    B, D, H, W = COUNT_GRID
    sol = None
    for d in range(9):
        for c in range(9):
            rest = n - 6 * c - 4 * d
            if rest >= 0 and rest % 9 == 0 and sol is None:
                sol = (rest // 18, (rest % 18) // 9, c, d)
    a, b, c, d = sol
    interior = [(y, x) for y in range(4, H - 3, 4) for x in range(2, W - 2, 4)]
    edges = [(y, x) for y in (0, H - 1) for x in range(4, W - 3, 4)]
    corners = [(z, y, x) for z in (0, 2, 4, 6, 8) for y in (0, H - 1) for x in (0, W - 1)]
    assert a + b <= len(interior) and c <= len(edges) and d <= len(corners), (n, sol)
    rows = []
    for i in range(a):
        rows.append((0, (1, 3, 5, 7)[i % 4]) + interior[i])
    for i in range(b):
        rows.append((0, (0, 2, 4, 6, 8)[i % 5]) + interior[a + i])
    for i in range(c):
        rows.append((0, (8, 6, 4, 2, 0)[i % 5]) + edges[i])
    for i in range(d):
        rows.append((0,) + corners[i])
    return Case(f"count_{n}", B, D, H, W, _shuffled(rows, 100 + n))


def _k_case(k):
    B, D, H, W = 2, 10, 40, 44
    return Case(f"k_{k}", B, D, H, W, _random_cells(B, D, H, W, k, 200 + k))


def _lattice():
    B, D, H, W = 2, 10, 132, 144
    rows = [(b, z, y, x) for b in range(B) for z in (1, 5) for y in range(1, H, 3) for x in range(1, W, 3)]
    return Case("lattice", B, D, H, W, _shuffled(rows, 15))


def _scan_carry():
    B, D, H, W = 2, 4, 400, 352
    return Case("scan_carry", B, D, H, W, _random_cells(B, D, H, W, 4000, 16))


_BUILDERS = {"full_block": _full_block, "corners_faces": _corners_faces, "batch_seam": _batch_seam,
             "one_item_empty": _one_item_empty, "single": _single, "empty": _empty, "depth_parity": _depth_parity,
             "lattice": _lattice, "scan_carry": _scan_carry}
_BUILDERS.update({f"count_{n}": functools.partial(_count_case, n) for n in COUNT_TARGETS})
_BUILDERS.update({f"k_{k}": functools.partial(_k_case, k) for k in K_TARGETS})

ALL_IDS = ("full_block", "corners_faces", "batch_seam", "one_item_empty", "single", "empty", "depth_parity") + \
    tuple(f"count_{n}" for n in COUNT_TARGETS) + tuple(f"k_{k}" for k in K_TARGETS) + ("lattice", "scan_carry")
GEMM_IDS = tuple(i for i in ALL_IDS if i != "scan_carry")                    # everything but the list-only case
LAYER_IDS = tuple(i for i in GEMM_IDS if i != "lattice")                     # ... with a dense float64 oracle
BACKWARD_IDS = ("full_block", "corners_faces", "batch_seam", "depth_parity", "k_255", "k_256", "k_257", "single")


@functools.lru_cache(maxsize=None)
def case(case_id):
    c = _BUILDERS[case_id]()
    coord = np.ascontiguousarray(c.coord, dtype=np.int64).reshape(-1, 4)
    coord.setflags(write=False)
    return c._replace(coord=coord)


def occupancy(c):
    """(B, 1, D, H, W) float64, 1 at every occupied cell"""
    occ = torch.zeros((c.B, 1, c.D, c.H, c.W), dtype=torch.float64)
    co = torch.from_numpy(np.array(c.coord))
    occ[co[:, 0], 0, co[:, 1], co[:, 2], co[:, 3]] = 1.0
    return occ


@functools.lru_cache(maxsize=None)
def oracle(case_id):
    """-> (sites int64 (n,4) [b, d, h, w] ascending, taps int64 (B, Do, H, W): occupied cells in every site's window)"""
    c = case(case_id)
    taps = F.conv3d(occupancy(c), torch.ones((1, 1) + KERNEL, dtype=torch.float64), None, STRIDE, PAD)[:, 0]
    taps = taps.round().long().numpy()
    sites = np.argwhere(taps > 0).astype(np.int64)           # argwhere: row-major = ascending linear order
    sites.setflags(write=False)
    taps.setflags(write=False)
    return sites, taps


def list_cap(c):
    """capacity of the active-site list as engine.first_layer_forward_sparse / the executor size it"""
    Do, Ho, Wo = out_dims(c.D, c.H, c.W)
    return max(1, min(c.B * Do * Ho * Wo, PER_VOXEL * len(c.coord)))


def scatter64(c, rows):
    """(K, C) rows -> dense float64 (B, C, D, H, W) with the rows at the case's cells"""
    rows = rows.double()
    dense = torch.zeros((c.B, c.D, c.H, c.W, rows.shape[1]), dtype=torch.float64)
    co = torch.from_numpy(np.array(c.coord))
    dense[co[:, 0], co[:, 1], co[:, 2], co[:, 3]] = rows
    return dense.permute(0, 4, 1, 2, 3).contiguous()


def single_tap(case_id):
    """for a case in which every active site sees exactly ONE voxel (proved by the host test: oracle max == 1):
    -> (voxel index (n,), tap index (n,)) of that one contribution per site of oracle(case_id)[0].  Read off two more
    convolutions, not off index arithmetic: a grid holding v + 1 at voxel v's cell under the all-ones kernel gives v + 1
    at the site, the occupancy under a kernel holding t + 1 at tap t gives t + 1 (one live term each: exact)."""
    c = case(case_id)
    sites, taps = oracle(case_id)
    assert taps.max() <= 1
    label = scatter64(c, torch.arange(1, len(c.coord) + 1, dtype=torch.float64).view(-1, 1))
    vox = F.conv3d(label, torch.ones((1, 1) + KERNEL, dtype=torch.float64), None, STRIDE, PAD)[:, 0]
    tapk = torch.arange(1, 28, dtype=torch.float64).view((1, 1) + KERNEL)
    tap = F.conv3d(occupancy(c), tapk, None, STRIDE, PAD)[:, 0]
    idx = tuple(sites.T)
    return vox.round().long().numpy()[idx] - 1, tap.round().long().numpy()[idx] - 1
