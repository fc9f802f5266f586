"""NumPy / plain-Python restatement of the true-IoU target assignment — the reference
tests/test_assign_host.py and tests/test_gpu_assign.py hold csrc/targets_iou.hip and voxelnet_amd/targets.py against.  It
shares no code with either: the rotated IoU is tests/eval_ref.iou_pair, the stand-up IoU is the few lines below.

Box = (x, y, z, h, w, l, r), float64.  IoU(n,k) of anchor n and ground truth k:
  "standup": the axis-aligned hulls x +- hx, y +- hy, hx = (l|cos r| + w|sin r|)/2, hy = (l|sin r| + w|cos r|)/2, areas
             without "+1", 0 when the hulls do not overlap; the overlap along an axis is written from the centres,
             min(h + h' - |c' - c|, 2 min(h, h')): anchors that all contain a box's hull along x tie EXACTLY;
  "rotated": the BEV IoU of the two rotated footprints (0 for a box with a non-finite field or h, w, l <= 0).
m_n = max_k IoU(n,k) at its smallest k = k_n;  M_k = max_n IoU(n,k) at its smallest n = n_k.
matched[n] = k_n if m_n >= pos_iou, else the smallest k with n_k == n and M_k > 0, else -1;  pos = matched >= 0;
neg = m_n < neg_iou and not pos; every anchor of a sample without a box is negative.  Regression targets: the reference's
seven expressions (utils.py:390-470) on the matched box, float64 rounded to float32, zeros elsewhere."""
import math

import numpy as np

import eval_ref as R

KINDS = ("standup", "rotated")


def hull(q):
    """(half width, half height) of the axis-aligned hull of the rotated footprint"""
    c, s = abs(math.cos(q[6])), abs(math.sin(q[6]))
    return (q[5] * c + q[4] * s) / 2, (q[5] * s + q[4] * c) / 2


def overlap(ca, ha, cg, hg):
    """length of [ca - ha, ca + ha] & [cg - hg, cg + hg], from the centres -> (length, whether one interval contains the
    other: the length is then 2 min(ha, hg) whatever the centres are)"""
    free, full = (ha + hg) - abs(cg - ca), 2.0 * min(ha, hg)
    return min(free, full), not free < full


def standup_terms(a, g):
    """-> (iw, ih, x saturated, y saturated, area of a's hull, area of g's hull)"""
    (ax, ay), (gx, gy) = hull(a), hull(g)
    iw, sx = overlap(a[0], ax, g[0], gx)
    ih, sy = overlap(a[1], ay, g[1], gy)
    return iw, ih, sx, sy, (2.0 * ax) * (2.0 * ay), (2.0 * gx) * (2.0 * gy)


def standup_iou(a, g):
    iw, ih, _, _, area_a, area_g = standup_terms(a, g)
    if not (iw > 0 and ih > 0):
        return 0.0
    inter = iw * ih
    v = inter / ((area_a + area_g) - inter)
    return v if v > 0 else 0.0


def same_by_construction(kind, a0, a1, g):
    """whether IoU(a0, g) == IoU(a1, g) in every implementation of the rules, whatever its rounding: a1 is a copy of a0; or,
    stand-up kind, the two anchors have one size and rotation and along each axis either the same centre or a saturated
    overlap (one hull contains the other: the overlap is 2 min(h, h'), the position does not enter)"""
    if np.array_equal(a0, a1):
        return True
    if kind != "standup" or not np.array_equal(a0[3:], a1[3:]):
        return False
    t0, t1 = standup_terms(a0, g), standup_terms(a1, g)
    return all((t0[2 + i] and t1[2 + i]) or a0[i] == a1[i] for i in range(2))


def iou_table(anchors, boxes, kind):
    """anchors (N,7), boxes (G,7) float64 -> (N,G) float64.  A footprint and its hull lie within the half-diagonal of the
    centre along either axis, so a pair whose centres are further apart along x or along y than 1.05 x the two
    half-diagonals together (plus 1 cm) overlaps in neither kind: 0 without evaluating it, which keeps the plain-Python
    pair function affordable on 70,400 anchors."""
    assert kind in KINDS
    a = np.asarray(anchors, dtype=np.float64).reshape(-1, 7)
    g = np.asarray(boxes, dtype=np.float64).reshape(-1, 7)
    out = np.zeros((a.shape[0], g.shape[0]), dtype=np.float64)
    hd_a = 0.5 * np.hypot(a[:, 4], a[:, 5])
    for k in range(g.shape[0]):
        with np.errstate(invalid="ignore"):
            hd = 0.5 * math.hypot(g[k, 4], g[k, 5])
            far = np.maximum(np.abs(a[:, 0] - g[k, 0]), np.abs(a[:, 1] - g[k, 1])) > 1.05 * (hd_a + hd) + 0.01          # NaN: not far
        for n in np.flatnonzero(~far):
            out[n, k] = standup_iou(a[n], g[k]) if kind == "standup" else R.iou_pair(a[n], g[k])[0]
    return out


def encode(a, g, anchor_h):
    """(NumPy's log: a box with w = 0 that the stand-up kind matches encodes to -inf, as the device's log does)"""
    diag = math.sqrt(a[4] ** 2 + a[5] ** 2)
    with np.errstate(divide="ignore"):
        return [(g[0] - a[0]) / diag, (g[1] - a[1]) / diag, (g[2] - a[2]) / anchor_h, np.log(g[3] / a[3]), np.log(g[4] / a[4]),
                np.log(g[5] / a[5]), g[6] - a[6]]


def assign_sample(anchors, boxes, kind, pos_iou, neg_iou, anchor_h, iou=None):
    """one sample -> dict(pos (N,) bool, neg (N,) bool, matched (N,) int, targets (N,7) float32, iou (N,G))"""
    a = np.asarray(anchors, dtype=np.float64).reshape(-1, 7)
    g = np.asarray(boxes, dtype=np.float64).reshape(-1, 7)
    N, G = a.shape[0], g.shape[0]
    pos_iou, neg_iou = float(np.float32(pos_iou)), float(np.float32(neg_iou))          # the float arguments, widened
    iou = iou_table(a, g, kind) if iou is None else iou
    matched = np.full(N, -1, dtype=np.int64)
    m = np.zeros(N)
    if G:
        m = iou.max(axis=1)
        k_n = iou.argmax(axis=1)                      # first occurrence: the smallest k
        M = iou.max(axis=0)
        n_k = iou.argmax(axis=0)                      # the smallest n
        for k in range(G - 1, -1, -1):                # descending: the smallest k is written last
            if M[k] > 0:
                matched[n_k[k]] = k
        thr = m >= pos_iou
        matched[thr] = k_n[thr]
    pos = matched >= 0
    neg = ~pos if G == 0 else (m < neg_iou) & ~pos
    targets = np.zeros((N, 7), dtype=np.float32)
    for n in np.flatnonzero(pos):
        targets[n] = np.array(encode(a[n], g[matched[n]], anchor_h), dtype=np.float64).astype(np.float32)
    return dict(pos=pos, neg=neg, matched=matched, targets=targets, iou=iou)


def assign(anchors, boxes_per_sample, kind, pos_iou, neg_iou, anchor_h):
    return [assign_sample(anchors, b, kind, pos_iou, neg_iou, anchor_h) for b in boxes_per_sample]


def guard(anchors, boxes, iou, pos_iou, neg_iou, margin, kind):
    """-> the smallest gap of one sample's decisions, asserting that none lies within `margin`:
    no m_n within the margin of either threshold; no M_k in (0, margin]; every box's best IoU(., k) ahead of the second best
    by more than the margin, unless the runners-up within the margin tie with it BY CONSTRUCTION (same_by_construction: a
    tiled grid's copies, a stand-up plateau — their IoUs are equal bit for bit in any implementation, and the smallest n
    wins); the same for every anchor's best box where m_n >= pos_iou (copies of a box tie exactly; the smallest k wins)."""
    a = np.asarray(anchors, dtype=np.float64).reshape(-1, 7)
    g = np.asarray(boxes, dtype=np.float64).reshape(-1, 7)
    pos_iou, neg_iou = float(np.float32(pos_iou)), float(np.float32(neg_iou))
    if g.shape[0] == 0:
        return float("inf")
    m = iou.max(axis=1)
    gap = float(min(np.abs(m - pos_iou).min(), np.abs(m - neg_iou).min()))
    assert gap > margin, ("a best IoU at a threshold", gap)
    for k in range(g.shape[0]):
        col = iou[:, k]
        best, n0 = col.max(), int(col.argmax())
        if best == 0:
            continue
        assert best > margin, ("a box that barely touches its best anchor", k, best)
        gap = min(gap, float(best))
        for n in np.flatnonzero(col >= best - margin):
            assert col[n] == best and same_by_construction(kind, a[n0], a[n], g[k]), \
                ("two anchors tie for a box", k, n0, int(n), best - col[n])
        rest = col[col < best - margin]
        if rest.size:
            gap = min(gap, float(best - rest.max()))
    for n in np.flatnonzero(m >= pos_iou):
        row = iou[n]
        k0 = int(row.argmax())
        for k in np.flatnonzero(row >= m[n] - margin):
            assert np.array_equal(g[k], g[k0]), ("two boxes tie for an anchor", int(n), k0, int(k), m[n] - row[k])
        rest = row[row < m[n] - margin]
        if rest.size:
            gap = min(gap, float(m[n] - rest.max()))
    return gap
