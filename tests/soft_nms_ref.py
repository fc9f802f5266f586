"""Float64 plain-Python restatement of the rules of DESIGN.md section 1n — Soft-NMS (vn_box_soft_nms) — that
tests/test_soft_nms_host.py and tests/test_gpu_soft_nms.py hold csrc/soft_nms.hip and voxelnet_amd/predict.py against.  It
shares no code with the package: the rotated IoU is tests/eval_ref.iou_pair, as tests/tta_ref.py uses it.

Box = (x, y, z, h, w, l, r).  Besides the walk's result the reference returns what a test needs to know BEFORE it looks at a
device: per kept row the number of decays and a bound on the relative error of its score, and the guards' figures."""
import math

import numpy as np

import eval_ref as R

HARD, LINEAR, GAUSSIAN = 0, 1, 2
BEV, D3 = 0, 1
IOU_BAR = 1e-9          # the project's bar for a device IoU against this pair function (tests/test_gpu_detection_eval.py)


def _ok(q):
    return all(math.isfinite(float(v)) for v in q) and min(float(q[3]), float(q[4]), float(q[5])) > 0


def soft_nms(boxes, scores, n, method, metric, iou_thres, sigma, min_score, post_top_k, cache=None):
    """one sample: boxes (K,7) f32, scores (K,) f32, n valid rows (clamped to [0, K]) -> dict
      keep      the picked rows in pick order
      w         their working scores, float64, BEFORE the one rounding to float32
      decays    how many multiplications each of them had taken when it was picked
      bound     the sum over those decays of |d ln f / du| * IOU_BAR: the relative error a device whose IoUs are within IOU_BAR
                of this reference's may show in w (linear: 1 / (1 - u); gaussian: 2 u / sigma)
      gap1      guard 1: the smallest relative distance |w_best - w_second| / |w_best| over the picks whose best and runner-up are
                not an exact tie of two rows no decay has touched (inf: none)
      touched_ties   how many picks had an exact tie in which a decay had touched one of the two rows
      gap2      guard 2: the smallest |u - iou_thres| over the evaluated IoUs u > 0 (inf: none)
      floor_gap the smallest relative distance |w - min_score| / max(|min_score|, 1e-300) over the comparisons of a row that a decay
                has touched with min_score (an untouched row's comparison is exact in float32 and float64 alike)
    `cache`: a dict that keeps the pair IoUs of these boxes between calls (the six method x metric walks share most pairs).
    A pair whose centres are further apart than the four side lengths together is disjoint: 0 without the clipping."""
    b = np.asarray(boxes, dtype=np.float32).astype(np.float64).reshape(-1, 7)
    s32 = np.asarray(scores, dtype=np.float32).reshape(-1)
    K = b.shape[0]
    n = min(max(int(n), 0), K)
    cache = {} if cache is None else cache
    w = s32.astype(np.float64)
    live = np.zeros(K, dtype=bool)
    for j in range(n):
        live[j] = _ok(b[j]) and math.isfinite(float(s32[j]))
    decays, bound = np.zeros(K, dtype=np.int64), np.zeros(K, dtype=np.float64)
    out = dict(keep=[], w=[], decays=[], bound=[], gap1=math.inf, touched_ties=0, gap2=math.inf, floor_gap=math.inf)
    while True:
        cand = np.nonzero(live)[0]
        if cand.size == 0:
            break
        i = int(cand[np.argmax(w[cand])])          # (the first of equal maxima: the smaller row; -0.0 == +0.0 as numbers)
        wi = float(w[i])
        if decays[i] > 0:
            out["floor_gap"] = min(out["floor_gap"], abs(wi - min_score) / max(abs(min_score), 1e-300))
        if not wi >= min_score:
            break
        others = cand[cand != i]
        if others.size:
            r = int(others[np.argmax(w[others])])
            if w[r] == wi:
                out["touched_ties"] += int(decays[i] > 0 or decays[r] > 0)
            else:
                out["gap1"] = min(out["gap1"], abs(wi - float(w[r])) / abs(wi) if wi != 0 else math.inf)
        out["keep"].append(i)
        out["w"].append(wi)
        out["decays"].append(int(decays[i]))
        out["bound"].append(float(bound[i]))
        live[i] = False
        if len(out["keep"]) == post_top_k:
            break
        a = b[i]
        near = others[np.hypot(b[others, 0] - a[0], b[others, 1] - a[1]) <= a[4] + a[5] + b[others, 4] + b[others, 5]]
        for j in (int(v) for v in near):
            pair = cache.get((i, j))
            if pair is None:
                pair = cache[(i, j)] = R.iou_pair(a, b[j])
            u = pair[1] if metric == D3 else pair[0]
            if u > 0:
                out["gap2"] = min(out["gap2"], abs(u - iou_thres))
            if method == HARD:
                if not u <= iou_thres:
                    live[j] = False
            elif method == LINEAR:
                if u > iou_thres:
                    w[j] = w[j] * (1.0 - u)
                    decays[j] += 1
                    bound[j] += IOU_BAR / (1.0 - u) if u < 1.0 else math.inf
            else:
                if u > 0:
                    w[j] = w[j] * math.exp(-(u * u) / sigma)
                    decays[j] += 1
                    bound[j] += 2.0 * u / sigma * IOU_BAR
    return out
