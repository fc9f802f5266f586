"""NumPy restatement of the occlusion-consistent paste (vn_gt_paste_visible) — the arbiter of
the device kernels.  Written on its own from the rules; it shares no code with the package and takes only the
point-in-box test from tests/gtsample_ref.py.  Every float64 expression is elementwise and spelled as the rules write
it; the depth buffers are plain per-bin minima (a lexicographic sort for the owner, no packed keys, no atomics).
"""
from dataclasses import dataclass

import numpy as np

import gtsample_ref as R


@dataclass
class Grid:
    nu: int = 512
    nv: int = 64
    v_lo: float = -0.47
    v_hi: float = 0.10
    margin: float = 0.3
    min_visible: int = 5


def bin_depth(cloud, grid):
    """(N,4) float32 -> (has (N,) bool, bin (N,) int64 — -1 without a bin —, depth (N,) float64 = a)"""
    cloud = np.asarray(cloud, dtype=np.float32).reshape(-1, 4)
    px = cloud[:, 0].astype(np.float64)
    py = cloud[:, 1].astype(np.float64)
    pz = cloud[:, 2].astype(np.float64)
    nu, nv = int(grid.nu), int(grid.nv)
    v_lo = np.float64(grid.v_lo)
    v_scale = np.float64(nv) / (np.float64(grid.v_hi) - v_lo)
    with np.errstate(all="ignore"):
        ax, ay = np.abs(px), np.abs(py)
        first = ax >= ay
        a = np.where(first, ax, ay)
        face = np.where(first, np.where(px > 0, 0, 2), np.where(py > 0, 1, 3))
        u = np.where(first, py, px) / a
        v = pz / a
        has = np.isfinite(px) & np.isfinite(py) & np.isfinite(pz) & (a != 0)
        iu = np.minimum(np.floor((u + 1.0) * np.float64(nu // 2)), np.float64(nu - 1))
        iv = np.floor((v - v_lo) * v_scale)
        has &= (iv >= 0) & (iv < nv)
    idx = np.full(cloud.shape[0], -1, dtype=np.int64)
    idx[has] = (face[has] * nv + iv[has].astype(np.int64)) * nu + iu[has].astype(np.int64)
    return has, idx, a


def _nearest(n_bins, idx, depth, mask):
    """per-bin minimum depth over the rows of `mask` (inf where a bin has none)"""
    d = np.full(n_bins, np.inf)
    np.minimum.at(d, idx[mask], depth[mask])
    return d


def paste_visible(cloud, boxes, obj, offsets, grid, cap=None):
    """-> dict(out (cap,4) float32, count, visible (G,) int32, accepted (G,) bool, kept (G,) int32, stats (2,) int32,
    scene_keep (N,) bool, obj_keep (M,) bool, obj_visible (M,) bool)"""
    cloud = np.asarray(cloud, dtype=np.float32).reshape(-1, 4)
    obj = np.asarray(obj, dtype=np.float32).reshape(-1, 4)
    boxes = np.asarray(boxes, dtype=np.float64).reshape(-1, 7)
    offsets = np.asarray(offsets, dtype=np.int64).reshape(-1)
    n, m, g = len(cloud), len(obj), len(boxes)
    assert len(offsets) == g + 1 and offsets[0] == 0 and offsets[-1] == m and (np.diff(offsets) >= 0).all()
    owner = np.repeat(np.arange(g, dtype=np.int64), np.diff(offsets))
    n_bins = 4 * int(grid.nv) * int(grid.nu)
    margin = np.float64(grid.margin)

    inside = R.masks(cloud, boxes) if g else np.zeros((0, n), dtype=bool)
    s_nan = np.isnan(cloud[:, :3]).any(1)
    s_has, s_bin, s_depth = bin_depth(cloud, grid)
    o_nan = np.isnan(obj[:, :3]).any(1)
    o_has, o_bin, o_depth = bin_depth(obj, grid)

    # pass 1: the scene's depth buffer, without the rows inside any candidate's box
    d_scene = _nearest(n_bins, s_bin, s_depth, ~s_nan & s_has & ~inside.any(0))
    # pass 2: visible object points, acceptance
    front = np.where(o_has, d_scene[np.where(o_has, o_bin, 0)], np.inf)
    with np.errstate(invalid="ignore"):
        o_visible = ~o_nan & ~(o_has & (o_depth > front + margin))
    visible = np.bincount(owner[o_visible], minlength=g).astype(np.int32)
    accepted = visible >= int(grid.min_visible)
    # pass 3: the accepted objects' depth buffer with its owner — nearest first, the lower object on a tie
    cand = np.flatnonzero(o_visible & accepted[owner] & o_has) if m else np.zeros(0, dtype=np.int64)
    d_obj = np.full(n_bins, np.inf)
    own = np.full(n_bins, -1, dtype=np.int64)
    order = cand[np.lexsort((owner[cand], o_depth[cand]))]
    for j in order[::-1]:                      # walked backwards: the first of the order is written last and stays
        d_obj[o_bin[j]] = o_depth[j]
        own[o_bin[j]] = owner[j]
    # pass 4: keep flags
    boxed = inside[accepted].any(0) & ~s_nan if g else np.zeros(n, dtype=bool)
    sb = np.where(s_has, s_bin, 0)
    with np.errstate(invalid="ignore"):
        shadowed = ~s_nan & ~boxed & s_has & (own[sb] >= 0) & (s_depth > d_obj[sb] + margin)
    scene_keep = ~s_nan & ~boxed & ~shadowed
    ob = np.where(o_has, o_bin, 0)
    with np.errstate(invalid="ignore"):
        culled = o_has & (own[ob] >= 0) & (own[ob] != owner) & (o_depth > d_obj[ob] + margin)
    obj_keep = o_visible & accepted[owner] & ~culled if m else np.zeros(0, dtype=bool)
    kept = np.bincount(owner[obj_keep], minlength=g).astype(np.int32)
    # pass 5: the output
    cap = n + m if cap is None else cap
    out = np.full((cap, 4), np.nan, dtype=np.float32)
    k, mk = int(scene_keep.sum()), int(obj_keep.sum())
    out[:k] = cloud[scene_keep]
    out[k:k + mk] = obj[obj_keep]
    return dict(out=out, count=k + mk, visible=visible, accepted=accepted, kept=kept,
                stats=np.array([boxed.sum(), shadowed.sum()], dtype=np.int32), scene_keep=scene_keep, obj_keep=obj_keep,
                obj_visible=o_visible)


def offsets_of(entries):
    """[points arrays] -> (G+1,) int32 offsets"""
    off = np.zeros(len(entries) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(p) for p in entries])
    return off
