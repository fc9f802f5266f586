"""NumPy restatement of the anchor mask, sharing nothing with csrc/anchor_mask.hip or
voxelnet_amd/anchor_mask.py: the cell rectangles with the OTHER operation order, the counts by brute force (no prefix
sum anywhere in it) and, for grids where that is too slow, by np.cumsum in int64.  Every quantity is an integer: the
kernels are held to exact equality."""
import numpy as np

SNAP = 1e-9


def rect_q(anchors, grid):
    """the four un-snapped rectangle edges in cells, (N, 4) float64 [q0, q1, q2, q3] — half extents as
    0.5 |sin r| w + 0.5 |cos r| l and a multiplication by 1 / vx (the package divides, and halves the sum)"""
    a = np.asarray(anchors, dtype=np.float64).reshape(-1, 7)
    q = np.empty((a.shape[0], 4))
    ivx, ivy = 1.0 / float(grid.vx), 1.0 / float(grid.vy)
    for n, (x, y, _, _, w, l, r) in enumerate(a):
        ex = 0.5 * abs(np.sin(r)) * w + 0.5 * abs(np.cos(r)) * l
        ey = 0.5 * abs(np.cos(r)) * w + 0.5 * abs(np.sin(r)) * l
        q[n] = ((x + float(grid.ox) - ex) * ivx, (y + float(grid.oy) - ey) * ivy,
                (x + float(grid.ox) + ex) * ivx, (y + float(grid.oy) + ey) * ivy)
    return q


def boundary_gap(q):
    """per component: the distance to the nearest integer"""
    return np.abs(q - np.rint(q))


def rects(anchors, grid):
    """(N, 4) int32 [w0, h0, w1, h1]: inclusive, snapped, half-open footprint, clipped; [0, 0, -1, -1] for an anchor whose
    unclipped rectangle is empty or misses the grid"""
    q = rect_q(anchors, grid)
    out = np.empty((q.shape[0], 4), dtype=np.int32)
    H, W = int(grid.H), int(grid.W)
    for n in range(q.shape[0]):
        v = []
        for k in range(4):
            c = float(q[n, k])
            if not np.isfinite(c):
                v = None
                break
            i = float(np.rint(c))
            if abs(c - i) <= SNAP:
                c = i
            v.append(int(np.floor(c)) if k < 2 else int(np.ceil(c)) - 1)
        if v is None or v[2] < v[0] or v[3] < v[1] or v[2] < 0 or v[3] < 0 or v[0] > W - 1 or v[1] > H - 1:
            out[n] = (0, 0, -1, -1)
        else:
            out[n] = (max(v[0], 0), max(v[1], 0), min(v[2], W - 1), min(v[3], H - 1))
    return out


def valid_rows(coord, B, H, W):
    c = np.asarray(coord, dtype=np.int64).reshape(-1, 4)
    ok = (c[:, 0] >= 0) & (c[:, 0] < B) & (c[:, 2] >= 0) & (c[:, 2] < H) & (c[:, 3] >= 0) & (c[:, 3] < W)
    return c[ok]


def count_brute(coord, B, H, W, rect, pick=None):
    """count[b, n] by comparing every voxel's (h, w) with the rectangle; pick: only these anchors (-> (B, len(pick)))"""
    c = valid_rows(coord, B, H, W)
    rect = np.asarray(rect, dtype=np.int64)
    idx = np.arange(rect.shape[0]) if pick is None else np.asarray(pick)
    out = np.zeros((B, idx.shape[0]), dtype=np.int64)
    for b in range(B):
        h, w = c[c[:, 0] == b, 2], c[c[:, 0] == b, 3]
        for j, n in enumerate(idx):
            w0, h0, w1, h1 = rect[n]
            out[b, j] = int(np.count_nonzero((w >= w0) & (w <= w1) & (h >= h0) & (h <= h1)))
    return out


def count_cumsum(coord, B, H, W, rect):
    """the same counts through a summed-area table in int64 (for the full grids)"""
    c = valid_rows(coord, B, H, W)
    occ = np.zeros((B, H, W), dtype=np.int64)
    np.add.at(occ, (c[:, 0], c[:, 2], c[:, 3]), 1)
    S = np.zeros((B, H + 1, W + 1), dtype=np.int64)
    S[:, 1:, 1:] = occ.cumsum(axis=1).cumsum(axis=2)
    r = np.asarray(rect, dtype=np.int64)
    w0, h0, w1, h1 = np.maximum(r[:, 0], 0), np.maximum(r[:, 1], 0), np.minimum(r[:, 2], W - 1), np.minimum(r[:, 3], H - 1)
    live = (w1 >= w0) & (h1 >= h0)
    w0, h0, w1, h1 = (np.where(live, v, 0) for v in (w0, h0, w1, h1))
    cnt = S[:, h1 + 1, w1 + 1] - S[:, h0, w1 + 1] - S[:, h1 + 1, w0] + S[:, h0, w0]
    return np.where(live[None, :], cnt, 0)


def mask_of(count, threshold):
    return (np.asarray(count) > threshold).astype(np.uint8)


def masked_probs(probs, mask, layout):
    """probs (B, 2, h, w) float32, mask (B, N) uint8 in anchor order n = 2 s + a -> the copy with +0.0 at masked-out anchors:
    "flat": anchor n <-> probs[b].flat[n]; "site": anchor n <-> probs[b, a, s]"""
    B = probs.shape[0]
    m = np.asarray(mask).reshape(B, -1)
    if layout == "site":
        m = m.reshape(B, -1, 2).transpose(0, 2, 1)
    out = np.array(probs, dtype=np.float32, copy=True)
    flat = out.reshape(B, -1)
    flat[m.reshape(B, -1) == 0] = np.float32(0.0)
    return out
