"""Float64 NumPy / plain-Python restatement of the rules of DESIGN.md section 1m — the merge of the views' candidate pools
(vn_pool_merge) and box voting (vn_box_vote) — that tests/test_tta_host.py and tests/test_gpu_tta.py hold csrc/tta.hip and
voxelnet_amd/tta.py against.  It shares no code with the package: the rotated IoU is tests/eval_ref.iou_pair.

Box = (x, y, z, h, w, l, r); a view = (fy, angle, factor): the cloud was (x, y) -> (x, fy*y) -> turned by -angle -> times factor."""
import math

import numpy as np

import eval_ref as R

W_SCORE, W_SCORE_IOU = 0, 1
S_KEEP, S_VIEW_MEAN = 0, 1


def forward_box(box, fy, angle, factor):
    """what augment.draw_compose does to a label box under the view (its stages 2-4), float64"""
    x, y, z, h, w, l, r = (float(v) for v in box)
    y, r = fy * y, fy * r
    c, s = math.cos(angle), math.sin(angle)
    x, y, r = x * c + y * s, -(x * s) + y * c, r - angle
    return np.array([x * factor, y * factor, z * factor, h * factor, w * factor, l * factor, r], dtype=np.float64)


def inverse_box(box, fy, angle, factor):
    """a view's box back in the frame's own coordinates, float64; the yaw is not wrapped"""
    q = [float(v) / factor for v in box[:6]]
    c, s = math.cos(angle), math.sin(angle)
    X, Y = q[0] * c - q[1] * s, q[0] * s + q[1] * c
    r = float(box[6]) + angle
    return np.array([X, fy * Y, q[2], q[3], q[4], q[5], fy * r], dtype=np.float64)


def merge(boxes, scores, counts, views):
    """one sample: boxes (V,K,7) f32, scores (V,K) f32, counts (V,), views (V,3) -> (boxes (n,7) f32, scores (n,) f32, src (n,)
    int): the rows k < min(max(count, 0), K) of every view whose score is not NaN, descending by score (-0.0 == +0.0), equal
    scores by src = v*K + k ascending; every box through inverse_box and ONE rounding to float32 (the identity view: copied)"""
    boxes, scores = np.asarray(boxes, dtype=np.float32), np.asarray(scores, dtype=np.float32)
    V, K = scores.shape
    rows = []
    for v in range(V):
        for k in range(min(max(int(counts[v]), 0), K)):
            s = float(scores[v, k])
            if not math.isnan(s):
                rows.append((-s, v * K + k))          # (-(-0.0) == -(+0.0) as numbers: one score)
    rows.sort()
    ob, os_, src = np.zeros((len(rows), 7), np.float32), np.zeros(len(rows), np.float32), np.zeros(len(rows), np.int64)
    for t, (_, g) in enumerate(rows):
        v, k = divmod(g, K)
        fy, angle, factor = (float(a) for a in views[v])
        if fy == 1.0 and angle == 0.0 and factor == 1.0:
            ob[t] = boxes[v, k]
        else:
            ob[t] = inverse_box(boxes[v, k].astype(np.float64), fy, angle, factor).astype(np.float32)
        os_[t], src[t] = scores[v, k], g
    return ob, os_, src


def _ok(q):
    return all(math.isfinite(float(v)) for v in q) and min(float(q[3]), float(q[4]), float(q[5])) > 0


def vote(boxes, scores, n, keep, thres, weight_mode=W_SCORE_IOU, score_mode=S_KEEP, src=None, rows_per_view=None, V=1):
    """one sample: boxes (K,7) f32 in priority order, scores (K,) f32, n valid rows, keep = the kept row numbers in walk order
    -> dict(boxes (m,7) f64 BEFORE the rounding to float32, scores (m,) f32, members (m,) int, t (m,) the walk positions in
    output order, iou_gap = the smallest |IoU - thres| over the evaluated IoUs > 0, wrap_gap = the smallest
    | |d| - pi/2 | over the members)"""
    b = np.asarray(boxes, dtype=np.float32).astype(np.float64)
    s32 = np.asarray(scores, dtype=np.float32)
    n = min(max(int(n), 0), b.shape[0])
    rows, iou_gap, wrap_gap = [], math.inf, math.inf
    for t, i in enumerate(int(v) for v in keep):
        if not (0 <= i < n) or not _ok(b[i]):
            continue
        sw, sq, sd, members = 0.0, np.zeros(6), 0.0, 0
        best = {}
        far = np.hypot(b[:n, 0] - b[i, 0], b[:n, 1] - b[i, 1]) > b[:n, 4] + b[:n, 5] + b[i, 4] + b[i, 5]
        for j in range(n):
            if j == i:
                u = 1.0
            else:
                if far[j] or not _ok(b[j]):
                    continue
                u = R.iou_pair(b[i], b[j])[0]
                if u > 0:
                    iou_gap = min(iou_gap, abs(u - thres))
                if not u >= thres:
                    continue
            s = float(s32[j])
            w = s * u if weight_mode == W_SCORE_IOU else s
            dr = b[j, 6] - b[i, 6]
            d = dr - math.pi * math.floor(dr / math.pi + 0.5)
            wrap_gap = min(wrap_gap, abs(abs(d) - math.pi / 2))
            sw, sq, sd, members = sw + w, sq + w * b[j, :6], sd + w * d, members + 1
            view = 0
            if src is not None:
                view = int(src[j]) // int(rows_per_view) if int(src[j]) >= 0 else -1
            best[view] = max(best.get(view, -math.inf), float(s32[j]))
        out = np.concatenate([sq / sw, [b[i, 6] + sd / sw]]) if sw > 0 else b[i].copy()
        if score_mode == S_VIEW_MEAN:
            acc = 0.0
            for v in range(V):
                acc += best.get(v, 0.0)
            score = np.float32(acc / V)
        else:
            score = s32[i]
        rows.append((out, score, members, t))
    order = sorted(range(len(rows)), key=lambda a: (-float(rows[a][1]), rows[a][3]))
    return dict(boxes=np.array([rows[a][0] for a in order], dtype=np.float64).reshape(-1, 7),
                scores=np.array([rows[a][1] for a in order], dtype=np.float32),
                members=np.array([rows[a][2] for a in order], dtype=np.int64),
                t=np.array([rows[a][3] for a in order], dtype=np.int64), iou_gap=iou_gap, wrap_gap=wrap_gap)


# ------------------------------------------------------------------------------------------------ clustered scenes
def object_centres(n_obj):
    """n_obj (<= 168) object centres on a 6 m pitch inside the Car range: no two closer than 6 m"""
    slots = [(2.0 + 6.0 * ix, -39.0 + 6.0 * iy) for iy in range(14) for ix in range(12)]
    assert n_obj <= len(slots)
    return slots[:n_obj]


def clustered_pools(seed, V, B, K, views, per=25, counts=None):
    """V views' candidate pools of B samples, K rows per view: per object (object_centres) and view `per` candidates — the
    object's box jittered (centre 0.15 m, size 3 %, yaw 0.05 rad), every third turned by pi — seen through the view
    (forward_box), rounded to float32; scores uniform in [0.3, 1), each view's rows in descending score.  As many whole
    objects as fit K rows (at least one, cut to K).  -> boxes (V,B,K,7) f32, scores (V,B,K) f32, counts (V,B) int32 (the
    number of rows made, unless `counts` overrides it)"""
    rng = np.random.default_rng(seed)
    n_obj = max(1, K // per)
    boxes = np.zeros((V, B, K, 7), np.float32)
    scores = np.zeros((V, B, K), np.float32)
    cnt = np.zeros((V, B), np.int32)
    for b in range(B):
        objs = []
        for cx, cy in object_centres(n_obj):
            objs.append(np.array([cx + rng.uniform(-0.5, 0.5), cy + rng.uniform(-0.5, 0.5), -1.0 + rng.uniform(-0.2, 0.2),
                                  1.5 + rng.uniform(-0.1, 0.1), 1.6 + rng.uniform(-0.1, 0.1), 3.9 + rng.uniform(-0.3, 0.3),
                                  rng.uniform(-math.pi, math.pi)]))
        for v in range(V):
            fy, angle, factor = (float(a) for a in views[v])
            rows = []
            for o in objs:
                for c in range(per):
                    q = o.copy()
                    q[:2] += rng.normal(0.0, 0.15, 2)
                    q[2] += rng.normal(0.0, 0.05)
                    q[3:6] *= 1.0 + rng.normal(0.0, 0.03, 3)
                    q[6] += rng.normal(0.0, 0.05) + (math.pi if c % 3 == 2 else 0.0)
                    rows.append(forward_box(q, fy, angle, factor))
            rows = np.array(rows[:K])
            sc = np.sort(rng.uniform(0.3, 1.0, len(rows)).astype(np.float32))[::-1]
            rows = rows[rng.permutation(len(rows))]
            boxes[v, b, :len(rows)], scores[v, b, :len(rows)], cnt[v, b] = rows.astype(np.float32), sc, len(rows)
    return boxes, scores, (cnt if counts is None else np.asarray(counts, np.int32).reshape(V, B))
