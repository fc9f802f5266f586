"""NumPy / plain-Python restatement of the evaluation tail's three rules — the reference
tests/test_detect_host.py and tests/test_gpu_detect.py hold csrc/detect.hip and voxelnet_amd/predict.py against.  It shares
no code with predict.py: the selection is np.lexsort, the rotated IoU is tests/eval_ref.iou_pair, the stand-up rectangles
are oracle.targets.gt_standup_2d (as oracle/predict.py takes them).

Box = (x, y, z, h, w, l, r), float32 rows as the device stores them."""
import math

import numpy as np

import eval_ref as R
from oracle.targets import CLASSES, gt_standup_2d

STANDUP, ROTATED = 0, 1


def select(probs, score_thres, pre_top_k):
    """probs (N,) float32 -> the flat indices of the min(M, pre_top_k) candidates with p >= score_thres, descending by
    (score, flat index): equal scores take the LARGER index first; -0.0 == +0.0; a NaN is never a candidate"""
    p = np.asarray(probs, dtype=np.float32).reshape(-1)
    with np.errstate(invalid="ignore"):
        cand = np.where(p >= np.float32(score_thres))[0]
    order = np.lexsort((cand, p[cand] + np.float32(0.0)))          # ascending by score, then by index
    return cand[order[::-1][:pre_top_k]].astype(np.int64)


def decode(deltas, anchors, idx, cls_name="Car"):
    """utils.py:476-489 for the rows `idx` only: deltas (14,h,w) float32 read as (N,7) without a permute, anchors (..,7)
    float64 -> (len(idx),7) float32 (float64 arithmetic, float32 exp)"""
    a = np.asarray(anchors, dtype=np.float64).reshape(-1, 7)[idx]
    d = np.asarray(deltas, dtype=np.float32).reshape(-1, 7)[idx]
    diag = np.sqrt(a[:, 4] ** 2 + a[:, 5] ** 2)
    out = np.zeros((len(idx), 7), dtype=np.float32)
    out[:, 0] = d[:, 0] * diag + a[:, 0]
    out[:, 1] = d[:, 1] * diag + a[:, 1]
    out[:, 2] = d[:, 2] * CLASSES[cls_name]["h"] + a[:, 2]
    out[:, 3:6] = np.exp(d[:, 3:6]) * a[:, 3:6]
    out[:, 6] = d[:, 6] + a[:, 6]
    return out


def box_valid(q):
    return all(math.isfinite(float(v)) for v in q) and min(float(q[3]), float(q[4]), float(q[5])) > 0


def _standup_iou(rect, i, js):
    """utils.py:519-551 for the pairs (kept i, later rows js): float64 rectangles, areas without '+1' (oracle/predict.py)"""
    x1, y1, x2, y2 = rect[:, 0], rect[:, 1], rect[:, 2], rect[:, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        area = (x2 - x1) * (y2 - y1)
        w = np.maximum(np.minimum(x2[js], x2[i]) - np.maximum(x1[js], x1[i]), 0.0)
        h = np.maximum(np.minimum(y2[js], y2[i]) - np.maximum(y1[js], y1[i]), 0.0)
        inter = w * h
        return inter / ((area[js] - inter) + area[i])


def nms(boxes, mode, nms_thres, post_top_k, cache=None):
    """boxes (n,7) float32 in priority order -> (kept row numbers, the smallest |IoU - nms_thres| over the IoUs the walk
    evaluated (inf: none)).  Walk the rows in order; a row that is not suppressed is kept; a kept row i suppresses every
    later row j with not (IoU(i,j) <= nms_thres); stop at post_top_k kept.  ROTATED: an invalid row is never kept and
    suppresses nothing.  `cache`: a dict that keeps the rectangles and the rotated IoUs of these boxes between calls.
    A rotated pair whose centres are further apart than the four side lengths together (more than twice the sum of the
    half-diagonals) is disjoint: 0 without the clipping, so that the plain-Python pair function is affordable."""
    boxes = np.asarray(boxes, dtype=np.float32).reshape(-1, 7)
    n = boxes.shape[0]
    b64 = boxes.astype(np.float64)
    cache = {} if cache is None else cache
    if mode == STANDUP:
        if "rect" not in cache:
            b2 = np.zeros((n, 7))
            b2[:, [0, 1, 4, 5, 6]] = b64[:, [0, 1, 4, 5, 6]]
            with np.errstate(invalid="ignore"):
                cache["rect"] = gt_standup_2d(b2).astype(np.float64).reshape(-1, 4)
        rect = cache["rect"]
        alive = np.ones(n, dtype=bool)
    else:
        alive = np.array([box_valid(q) for q in b64], dtype=bool).reshape(n)
    keep, gap = [], float("inf")
    for i in range(n):
        if not alive[i]:
            continue
        keep.append(i)
        if len(keep) == post_top_k:
            break
        js = i + 1 + np.nonzero(alive[i + 1:])[0]
        if js.size == 0:
            continue
        if mode == STANDUP:
            iou = _standup_iou(rect, i, js)
        else:
            a = b64[i]
            far = np.hypot(b64[js, 0] - a[0], b64[js, 1] - a[1]) > a[4] + a[5] + b64[js, 4] + b64[js, 5]
            iou = np.zeros(js.size)
            for k in np.nonzero(~far)[0]:
                j = int(js[k])
                v = cache.get((i, j))
                if v is None:
                    v = cache[(i, j)] = R.iou_pair(a, b64[j])[0]
                iou[k] = v
        ok = ~np.isnan(iou)
        if ok.any():
            gap = min(gap, float(np.abs(iou[ok] - nms_thres).min()))
        with np.errstate(invalid="ignore"):
            alive[js[~(iou <= nms_thres)]] = False
    return keep, gap


def detect(probs, deltas, anchors, score_thres, pre_top_k, mode, nms_thres, post_top_k, cls_name="Car"):
    """one sample's maps -> (boxes (k,7) float32, scores (k,) float32): select, decode (with the class's anchor height),
    nms, gather"""
    idx = select(probs, score_thres, pre_top_k)
    boxes = decode(deltas, anchors, idx, cls_name)
    keep, _ = nms(boxes, mode, nms_thres, post_top_k)
    return boxes[keep], np.asarray(probs, dtype=np.float32).reshape(-1)[idx][keep]
