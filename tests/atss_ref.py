"""NumPy / plain-Python restatement of the ATSS target assignment (include/voxelnet_hip.h states the
rules) — the reference tests/test_atss_host.py and tests/test_gpu_atss.py hold csrc/targets_atss.hip and
voxelnet_amd/targets.py against.  It shares no code with either: the rotated IoU is tests/eval_ref.iou_pair, the stand-up IoU
and the encoding are tests/assign_ref's.

Anchor n = site * 2 + rotation, group a = anchors with n & 1 == a.  For a valid box k (all fields finite, h, w, l > 0):
  d2(n,k) = dx*dx + dy*dy, dx = x_n - x_k, dy = y_n - y_k;
  C_k = per group the min(top_k, N/2) anchors with the smallest (d2, n) (np.lexsort: equal d2 goes to the smaller n);
  v(n,k) = the IoU of `kind`;  mu = mean(v), sd = std(v, ddof=1) over C_k, t = mu + sd;
  k accepts n in C_k when v >= t, v > 0 and |u| <= l/2, |w'| <= w/2 (u = dx cos r + dy sin r, w' = -dx sin r + dy cos r);
  matched[n] = the accepting box of the largest v, the smallest k among equals, else -1; pos = matched >= 0; neg = ~pos;
  targets = assign_ref.encode on the matched box, float64 rounded to float32, zeros elsewhere;
  stats[k] = (mu, sd, t, number of anchors matched to k), zeros for an invalid box."""
import math

import numpy as np

import assign_ref as A
import eval_ref as R

KINDS = A.KINDS


def box_valid(q):
    return bool(np.all(np.isfinite(q)) and q[3] > 0 and q[4] > 0 and q[5] > 0)


def ranked(anchors, box):
    """-> per group the anchors' indices n in ascending (d2, n), and d2 (N,)"""
    a = np.asarray(anchors, dtype=np.float64).reshape(-1, 7)
    dx, dy = a[:, 0] - box[0], a[:, 1] - box[1]
    d2 = dx * dx + dy * dy
    out = []
    for g in range(2):
        n = np.arange(g, a.shape[0], 2)
        out.append(n[np.lexsort((n, d2[n]))])
    return out, d2


def pair_iou(a, g, kind):
    return A.standup_iou(a, g) if kind == "standup" else R.iou_pair(a, g)[0]


def local_offsets(a, g):
    """-> (|u| - l/2, |w'| - w/2) of anchor a's centre in box g's frame: both <= 0 is inside"""
    dx, dy = a[0] - g[0], a[1] - g[1]
    c, s = math.cos(g[6]), math.sin(g[6])
    return abs(dx * c + dy * s) - g[5] / 2, abs(-dx * s + dy * c) - g[4] / 2


def assign_sample(anchors, boxes, kind, top_k, anchor_h, order=None):
    """one sample -> dict(pos, neg (N,) bool, matched (N,) int, targets (N,7) float32, stats (G,4), cand: per box the candidates
    n (group 0 by rank, then group 1; empty for an invalid box), v: per box their IoUs, accept: per box the accepted mask).
    order: per box `ranked`'s first element, when the caller has it already."""
    assert kind in KINDS and 1 <= top_k <= 32
    a = np.asarray(anchors, dtype=np.float64).reshape(-1, 7)
    g = np.asarray(boxes, dtype=np.float64).reshape(-1, 7)
    N, G = a.shape[0], g.shape[0]
    assert N % 2 == 0
    K = min(top_k, N // 2)
    cand, vs, acc = [], [], []
    stats = np.zeros((G, 4))
    best_v = np.zeros(N)
    matched = np.full(N, -1, dtype=np.int64)
    for k in range(G):
        if not box_valid(g[k]):
            cand.append(np.zeros(0, dtype=np.int64)); vs.append(np.zeros(0)); acc.append(np.zeros(0, dtype=bool))
            continue
        groups = ranked(a, g[k])[0] if order is None else order[k]
        c = np.concatenate([groups[0][:K], groups[1][:K]])
        v = np.array([pair_iou(a[n], g[k], kind) for n in c], dtype=np.float64)
        mu, sd = float(v.mean()), float(v.std(ddof=1))
        t = mu + sd
        stats[k, :3] = mu, sd, t
        ok = np.zeros(c.size, dtype=bool)
        for i, n in enumerate(c):
            du, dw = local_offsets(a[n], g[k])
            ok[i] = v[i] >= t and v[i] > 0 and du <= 0 and dw <= 0
            if ok[i] and v[i] > best_v[n]:          # strict: the smallest k of the largest v
                best_v[n], matched[n] = v[i], k
        cand.append(c); vs.append(v); acc.append(ok)
    for k in range(G):
        stats[k, 3] = np.count_nonzero(matched == k)
    pos = matched >= 0
    targets = np.zeros((N, 7), dtype=np.float32)
    for n in np.flatnonzero(pos):
        targets[n] = np.array(A.encode(a[n], g[matched[n]], anchor_h), dtype=np.float64).astype(np.float32)
    return dict(pos=pos, neg=~pos, matched=matched, targets=targets, stats=stats, cand=cand, v=vs, accept=acc)


def guard(anchors, boxes, ref, top_k, margin):
    """asserts ON THE REFERENCE ALONE that no decision of one sample lies within `margin` -> dict of the smallest gaps:
    cut    the centre distance (metres) of a group's last candidate ahead of its first non-candidate, unless their |dx| and
           |dy| are bit-equal (d2 is then equal in any implementation and the smaller n wins);
    thr    |v - t| of every candidate (a box whose candidates all have IoU exactly 0 decides nothing by its threshold);
    edge   ||u| - l/2| and ||w'| - w/2| of every candidate;
    tie    an anchor accepted by two boxes: its best v ahead of the second, unless the two boxes are copies."""
    a = np.asarray(anchors, dtype=np.float64).reshape(-1, 7)
    g = np.asarray(boxes, dtype=np.float64).reshape(-1, 7)
    K = min(top_k, a.shape[0] // 2)
    gaps = dict(cut=math.inf, thr=math.inf, edge=math.inf, tie=math.inf)
    takers = {}
    for k in range(g.shape[0]):
        if not box_valid(g[k]):
            continue
        groups, d2 = ranked(a, g[k])
        for grp in groups:
            if grp.size > K:
                last, nxt = grp[K - 1], grp[K]
                same = all(abs(a[last, i] - g[k, i]) == abs(a[nxt, i] - g[k, i]) for i in range(2))
                if not same:
                    gap = math.sqrt(d2[nxt]) - math.sqrt(d2[last])
                    assert gap > margin, ("the candidate cut", k, int(last), int(nxt), gap)
                    gaps["cut"] = min(gaps["cut"], gap)
        c, v, t = ref["cand"][k], ref["v"][k], ref["stats"][k, 2]
        if v.any():
            gap = float(np.abs(v - t).min())
            assert gap > margin, ("an IoU at the box's threshold", k, gap)
            gaps["thr"] = min(gaps["thr"], gap)
        for i, n in enumerate(c):
            gap = min(abs(x) for x in local_offsets(a[n], g[k]))
            assert gap > margin, ("a centre on the footprint's edge", k, int(n), gap)
            gaps["edge"] = min(gaps["edge"], gap)
            if ref["accept"][k][i]:
                takers.setdefault(int(n), []).append((v[i], k))
    for n, lst in takers.items():
        lst.sort(key=lambda e: (-e[0], e[1]))
        for v2, k2 in lst[1:]:
            if np.array_equal(g[k2], g[lst[0][1]]):
                continue
            gap = lst[0][0] - v2
            assert gap > margin, ("two boxes tie for an anchor", n, lst[0][1], k2, gap)
            gaps["tie"] = min(gaps["tie"], gap)
    return gaps
