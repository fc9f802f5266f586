"""NumPy / plain-Python restatement of the SimOTA target assignment (include/voxelnet_hip.h states the
rules) — the reference tests/test_ota_host.py and tests/test_gpu_ota.py hold csrc/targets_ota.hip and voxelnet_amd/targets.py
against.  It shares no code with either: the rotated IoU is tests/eval_ref.iou_pair, the decode is tests/iou_loss_ref.decode's
seven expressions on NumPy float64, the encoding is tests/assign_ref.encode, the rankings are np.lexsort.

Anchor n = site * 2 + a.  probs (2, S) and deltas (14, S) float32 of one sample in the site layout: anchor (s, a) has
p = probs[a, s] and d_j = deltas[7a + j, s].  For a valid box k (all fields finite, h, w, l > 0), dx = x_n - x_k, dy = y_n - y_k,
u = dx cos r + dy sin r, w' = -dx sin r + dy cos r:
  in_box = |u| <= l/2 and |w'| <= w/2;  in_ctr = |dx| <= radius and |dy| <= radius;  C_k = {n : in_box or in_ctr};
  v(n,k) = iou_pair(decode(d, anchor n), gt_k)[metric];
  cost = -log(pc) + iou_weight * -log(v + 1e-8) + (0 if in_box and in_ctr else 1e5), pc = p clamped to [1e-12, 1], NaN -> 1e-12;
  m = min(q, |C_k|); sum_k = the m largest v, added in descending (v, then ascending n) order; dyn_k = max(1, floor(sum_k));
  k selects the dyn_k smallest (cost, n) of C_k; matched[n] = the selecting box of the smallest cost, the smallest k among
  equals, else -1; pos = matched >= 0; neg = ~pos; targets = assign_ref.encode on the matched box rounded to float32;
  stats[k] = (|C_k|, sum_k, dyn_k, cost of the last selected candidate, anchors matched to k), zeros without a candidate."""
import math

import numpy as np

import assign_ref as A
import eval_ref as R

METRICS = ("bev", "3d")
OUTSIDE = 1e5
V_FLOOR = 1e-4          # guard: a candidate's v is exactly 0 or at least this (near 0 the term -log(v + 1e-8) magnifies v's last bits)


def box_valid(q):
    return bool(np.all(np.isfinite(q)) and q[3] > 0 and q[4] > 0 and q[5] > 0)


def offsets(a, g, radius):
    """anchors a (N,7), box g -> (|u| - l/2, |w'| - w/2, |dx| - radius, |dy| - radius), each (N,): <= 0 is inside"""
    dx, dy = a[:, 0] - g[0], a[:, 1] - g[1]
    c, s = math.cos(g[6]), math.sin(g[6])
    return np.abs(dx * c + dy * s) - g[5] / 2, np.abs(-(dx * s) + dy * c) - g[4] / 2, np.abs(dx) - radius, np.abs(dy) - radius


def decode(d, a):
    """iou_loss_ref.decode's expressions on float64 scalars: regression values d (7,) on anchor a (7,) -> the box"""
    diag = math.sqrt(a[4] * a[4] + a[5] * a[5])
    with np.errstate(over="ignore"):
        e = np.exp(np.asarray(d[3:6], dtype=np.float64))
    return [d[0] * diag + a[0], d[1] * diag + a[1], d[2] * a[3] + a[2], e[0] * a[3], e[1] * a[4], e[2] * a[5], d[6] + a[6]]


def pair_values(anchors, boxes, probs, deltas, radius):
    """what does not depend on (metric, q, iou_weight), per box of one sample: dict(n: the candidates ascending, both: in_box and
    in_ctr, v: (|C|, 2) the BEV and 3D IoU of decoded prediction and box, p: their probs widened); None for an invalid box"""
    a = np.asarray(anchors, dtype=np.float64).reshape(-1, 7)
    g = np.asarray(boxes, dtype=np.float64).reshape(-1, 7)
    S = a.shape[0] // 2
    probs = np.asarray(probs).reshape(2, S)
    deltas = np.asarray(deltas).reshape(14, S)
    assert probs.dtype == np.float32 and deltas.dtype == np.float32 and a.shape[0] % 2 == 0
    out = []
    for k in range(g.shape[0]):
        if not box_valid(g[k]):
            out.append(None)
            continue
        eu, ew, ex, ey = offsets(a, g[k], radius)
        in_box, in_ctr = (eu <= 0) & (ew <= 0), (ex <= 0) & (ey <= 0)
        n = np.flatnonzero(in_box | in_ctr)
        v = np.zeros((n.size, 2))
        for i, ni in enumerate(n):
            s, r = divmod(int(ni), 2)
            d = deltas[7 * r:7 * r + 7, s].astype(np.float64)
            v[i] = R.iou_pair(decode(d, a[ni]), g[k])
        out.append(dict(n=n, both=(in_box & in_ctr)[n], v=v, p=probs[n % 2, n // 2].astype(np.float64)))
    return out


def cost_of(p, v, both, iou_weight):
    pc = 1e-12 if not p >= 1e-12 else min(p, 1.0)          # (a NaN p too)
    return -math.log(pc) + iou_weight * (-math.log(v + 1e-8)) + (0.0 if both else OUTSIDE)


def assign_sample(anchors, boxes, pairs, metric, q, iou_weight, anchor_h):
    """one sample, `pairs` = pair_values(...) -> dict(pos, neg (N,) bool, matched (N,) int, targets (N,7) float32, stats (G,5),
    and per box (empty for one without candidates): cand — its candidates n ascending, v, cost, order — the candidates' positions
    in ascending (cost, n), sel — the selected anchors in that order)"""
    assert metric in METRICS and 1 <= q <= 16
    a = np.asarray(anchors, dtype=np.float64).reshape(-1, 7)
    g = np.asarray(boxes, dtype=np.float64).reshape(-1, 7)
    N, G, col = a.shape[0], g.shape[0], METRICS.index(metric)
    stats = np.zeros((G, 5))
    cand, vs, costs, orders, sels = [], [], [], [], []
    best = {}          # n -> (cost, k)
    for k in range(G):
        pk = pairs[k]
        if pk is None or pk["n"].size == 0:
            cand.append(np.zeros(0, dtype=np.int64)); vs.append(np.zeros(0)); costs.append(np.zeros(0))
            orders.append(np.zeros(0, dtype=np.int64)); sels.append(np.zeros(0, dtype=np.int64))
            continue
        n, v = pk["n"], np.ascontiguousarray(pk["v"][:, col])
        cost = np.array([cost_of(float(p), float(x), bool(b), iou_weight) for p, x, b in zip(pk["p"], v, pk["both"])])
        m = min(q, n.size)
        total = 0.0
        for i in np.lexsort((n, -v))[:m]:
            total += float(v[i])
        dyn_k = max(1, int(math.floor(total)))
        assert dyn_k <= m
        order = np.lexsort((n, cost))
        sel = order[:dyn_k]
        stats[k, :4] = n.size, total, dyn_k, cost[sel[-1]]
        for i in sel:
            key = (float(cost[i]), k)
            if int(n[i]) not in best or key < best[int(n[i])]:
                best[int(n[i])] = key
        cand.append(n); vs.append(v); costs.append(cost); orders.append(order); sels.append(n[sel])
    matched = np.full(N, -1, dtype=np.int64)
    for n, (_, k) in best.items():
        matched[n] = k
    for k in range(G):
        stats[k, 4] = np.count_nonzero(matched == k)
    pos = matched >= 0
    targets = np.zeros((N, 7), dtype=np.float32)
    for n in np.flatnonzero(pos):
        targets[n] = np.array(A.encode(a[n], g[matched[n]], anchor_h), dtype=np.float64).astype(np.float32)
    return dict(pos=pos, neg=~pos, matched=matched, targets=targets, stats=stats, cand=cand, v=vs, cost=costs, order=orders, sel=sels)


def _inputs_equal(a, probs, deltas, n0, n1):
    """whether anchors n0 and n1 are bit-equal copies with bit-equal predictions: their costs for any box are then equal in
    every implementation, and the smaller n ranks first"""
    S = a.shape[0] // 2
    (s0, r0), (s1, r1) = divmod(n0, 2), divmod(n1, 2)
    p = np.asarray(probs).reshape(2, S).view(np.uint32)
    d = np.asarray(deltas).reshape(14, S).view(np.uint32)
    return bool(np.array_equal(a[n0], a[n1]) and p[r0, s0] == p[r1, s1] and np.array_equal(d[7 * r0:7 * r0 + 7, s0], d[7 * r1:7 * r1 + 7, s1]))


def guard(anchors, boxes, probs, deltas, ref, radius, margin):
    """asserts ON THE REFERENCE ALONE that no decision of one sample lies within `margin` -> dict of the smallest gaps:
    edge    ||u| - l/2| and ||w'| - w/2| of EVERY anchor, candidate or not (membership of C_k and the 1e5 term hang on them),
            wherever the test's other offset does not already say "outside";
    radius  ||dx| - radius| and ||dy| - radius| likewise;
    floor   sum_k from the nearest integer — unless sum_k is exactly 0: every term is then the pair function's exact 0;
    cut     the last selected cost ahead of the first unselected one, unless the two anchors' inputs are bit-equal copies;
    tie     an anchor selected by two boxes: its smallest cost ahead of the next, unless the two boxes are copies.
    And every candidate's v, in both metrics, is exactly 0 or >= V_FLOOR."""
    a = np.asarray(anchors, dtype=np.float64).reshape(-1, 7)
    g = np.asarray(boxes, dtype=np.float64).reshape(-1, 7)
    gaps = dict(edge=math.inf, radius=math.inf, floor=math.inf, cut=math.inf, tie=math.inf)
    takers = {}
    for k in range(g.shape[0]):
        if not box_valid(g[k]):
            continue
        eu, ew, ex, ey = offsets(a, g[k], radius)
        # (an offset decides something only where the test's other offset does not already say "outside")
        for name, e, other in (("edge", eu, ew), ("edge", ew, eu), ("radius", ex, ey), ("radius", ey, ex)):
            e = np.abs(e[other <= margin])
            if e.size:
                gap = float(e.min())
                assert gap > margin, ("an anchor on the " + name, k, gap)
                gaps[name] = min(gaps[name], gap)
        n, v, cost, order = ref["cand"][k], ref["v"][k], ref["cost"][k], ref["order"][k]
        if n.size == 0:
            continue
        assert np.all((v == 0) | (v >= V_FLOOR)), ("a candidate's IoU in (0, V_FLOOR)", k, float(v[(v > 0) & (v < V_FLOOR)].min()))
        total, dyn_k = ref["stats"][k, 1], int(ref["stats"][k, 2])
        if total != 0.0:
            gap = abs(total - round(total))
            assert gap > margin, ("sum_k on an integer", k, total)
            gaps["floor"] = min(gaps["floor"], gap)
        if dyn_k < n.size:
            last, nxt = order[dyn_k - 1], order[dyn_k]
            if not _inputs_equal(a, probs, deltas, int(n[last]), int(n[nxt])):
                gap = float(cost[nxt] - cost[last])
                assert gap > margin, ("the selection cut", k, int(n[last]), int(n[nxt]), gap)
                gaps["cut"] = min(gaps["cut"], gap)
        for i in order[:dyn_k]:
            takers.setdefault(int(n[i]), []).append((float(cost[i]), k))
    for n, lst in takers.items():
        lst.sort()
        for c2, k2 in lst[1:]:
            if np.array_equal(g[k2], g[lst[0][1]]):
                continue
            gap = c2 - lst[0][0]
            assert gap > margin, ("two boxes tie for an anchor", n, lst[0][1], k2, gap)
            gaps["tie"] = min(gaps["tie"], gap)
    return gaps
