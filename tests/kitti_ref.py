"""Float64 NumPy / plain-Python restatement of the image-plane scoring rules — the reference
tests/test_kitti_eval_host.py and tests/test_gpu_kitti_eval.py hold voxelnet_amd/evaluate.py's KittiDetectionEvaluator and
csrc/eval.hip's vn_boxes_to_image / vn_eval_match_image against.  It shares no code with evaluate.py; the rotated IoU is
tests/eval_ref.py's.

Box = (x, y, z, h, w, l, r), lidar frame.  Calibration of a frame = (P2 (3,4), Tr_velo_to_cam (4,4), R0_rect (4,4))."""
import math

import numpy as np

import eval_ref as R

DIFFS = ("all", "easy", "moderate", "hard")
THRES = {"Car": 0.7, "Pedestrian": 0.5, "Cyclist": 0.5}
NEIGHBOURS = {"Car": ("Van",), "Pedestrian": ("Person_sitting",), "Cyclist": ()}
MIN_HEIGHT = {"all": None, "easy": 40.0, "moderate": 25.0, "hard": 25.0}
_FILTER = {"easy": (40.0, 0, 0.15), "moderate": (25.0, 1, 0.30), "hard": (25.0, 2, 0.50)}
IMAGE_HW = (375, 1242)
METRICS = ("bev", "3d", "bbox")

# the mean calibration: targets.py's two matrices (written out again) and the mean P2 = tests/golden/fov_crop.npz's `P`
MEAN_TR = np.array([[7.49916597e-03, -9.99971248e-01, -8.65110297e-04, -6.71807577e-03],
                    [1.18652889e-02, 9.54520517e-04, -9.99910318e-01, -7.33152811e-02],
                    [9.99882833e-01, 7.49141178e-03, 1.18719929e-02, -2.78557062e-01],
                    [0, 0, 0, 1]])
MEAN_R0 = np.array([[0.99992475, 0.00975976, -0.00734152, 0], [-0.0097913, 0.99994262, -0.00430371, 0],
                    [0.00729911, 0.0043753, 0.99996319, 0], [0, 0, 0, 1]])
MEAN_P2 = np.array([[np.float32(7.1978711e+02), 0, np.float32(6.0846301e+02), np.float32(4.4953876e+01)],
                    [0, np.float32(7.1978711e+02), np.float32(1.7454510e+02), np.float32(1.0668550e-01)],
                    [0, 0, 1, np.float32(3.0106471e-03)]], dtype=np.float64)
MEAN_CALIB = (MEAN_P2, MEAN_TR, MEAN_R0)


def wrap(a):
    """into (-pi, pi]"""
    while a > math.pi:
        a -= 2 * math.pi
    while a <= -math.pi:
        a += 2 * math.pi
    return a


def seam_distance(a):
    """how far the angle a (before wrapping) is from the seam pi + 2 k pi"""
    t = (a - math.pi) % (2 * math.pi)
    return min(t, 2 * math.pi - t)


def lidar_to_cam(calib):
    _, Tr, R0 = calib
    return np.asarray(R0, dtype=np.float64) @ np.asarray(Tr, dtype=np.float64)


# ------------------------------------------------------------------------------------------------- projection
def project_box(box, calib=MEAN_CALIB, image_hw=IMAGE_HW):
    """one lidar box -> dict: row (12: alpha x1 y1 x2 y2 h w l xc yc zc ry), on (bool), and what the guards look at:
    depths (8,), raw (x1, y1, x2, y2 before the on-image decision), angles (the two pre-wrap angles).
    A box with a non-finite field or a non-positive size: twelve zeros, off.  A box off the image: 2D fields zero."""
    b = [float(v) for v in box]
    out = {"row": np.zeros(12), "on": False, "depths": None, "raw": None, "angles": None}
    if not all(math.isfinite(v) for v in b) or min(b[3], b[4], b[5]) <= 0:
        return out
    x, y, z, h, w, l, r = b
    M = lidar_to_cam(calib)[:3]
    P2 = np.asarray(calib[0], dtype=np.float64)
    c = M @ np.array([x, y, z, 1.0])
    ry_raw = -r - math.pi / 2
    ry = wrap(ry_raw)
    al_raw = ry - math.atan2(c[0], c[2])
    alpha = wrap(al_raw)
    us, vs, ds = [], [], []
    for dz in (0.0, h):
        for sx in (1, -1):
            for sy in (1, -1):
                px = x + sx * l / 2 * math.cos(r) - sy * w / 2 * math.sin(r)
                py = y + sx * l / 2 * math.sin(r) + sy * w / 2 * math.cos(r)
                q = P2 @ np.append(M @ np.array([px, py, z + dz, 1.0]), 1.0)
                ds.append(q[2])
                us.append(q[0] / q[2] if q[2] != 0 else math.inf)
                vs.append(q[1] / q[2] if q[2] != 0 else math.inf)
    H, W = image_hw
    out["row"][[0, 5, 6, 7, 8, 9, 10, 11]] = [alpha, h, w, l, c[0], c[1], c[2], ry]
    out["depths"] = np.array(ds)
    out["angles"] = (ry_raw, al_raw)
    if min(ds) > 0.1:
        x1, y1, x2, y2 = max(min(us), 0.0), max(min(vs), 0.0), min(max(us), W - 1.0), min(max(vs), H - 1.0)
        out["raw"] = (x1, y1, x2, y2)
        if x2 > x1 and y2 > y1:
            out["on"] = True
            out["row"][1:5] = [x1, y1, x2, y2]
    return out


def iou_2d(a, b):
    """two rectangles (x1, y1, x2, y2): areas without '+1'; 0 when the union is <= 0"""
    iw = min(a[2], b[2]) - max(a[0], b[0])
    ih = min(a[3], b[3]) - max(a[1], b[1])
    inter = iw * ih if iw > 0 and ih > 0 else 0.0
    union = (a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - inter
    return inter / union if union > 0 else 0.0


def dontcare_overlap(det, regions):
    """the largest area(det & D) / area(det) over the regions (0 without one)"""
    area = (det[2] - det[0]) * (det[3] - det[1])
    best = 0.0
    for d in regions:
        iw = min(det[2], d[2]) - max(det[0], d[0])
        ih = min(det[3], d[3]) - max(det[1], d[1])
        if iw > 0 and ih > 0 and area > 0:
            best = max(best, iw * ih / area)
    return best


# ------------------------------------------------------------------------------------------------ ground truths
def frame_ground_truth(lines, cls_name="Car", diffs=DIFFS, calib=MEAN_CALIB):
    """-> dict: boxes (G,7) lidar by the FRAME's calibration (r = wrap(-ry - pi/2), no snap), flags (n_diff,G) bool
    (True = ignored), bbox (G,4), alpha (G,), dontcare (D,4)"""
    inv = np.linalg.inv(lidar_to_cam(calib))
    boxes, flags, bbox, alpha, dc = [], [], [], [], []
    for line in lines:
        f = line.split()
        name = f[0]
        if name == "DontCare":
            dc.append([float(f[4]), float(f[5]), float(f[6]), float(f[7])])
            continue
        if name == cls_name:
            trunc, occ, height = float(f[1]), float(f[2]), float(f[7]) - float(f[5])
            row = []
            for d in diffs:
                if d == "all":
                    row.append(False)
                else:
                    hmin, omax, tmax = _FILTER[d]
                    row.append(not (height >= hmin and occ <= omax and trunc <= tmax))
        elif name in NEIGHBOURS[cls_name]:
            row = [True] * len(diffs)
        else:
            continue
        h, w, l, x, y, z, ry = (float(v) for v in f[8:15])
        p = inv @ np.array([x, y, z, 1.0])
        boxes.append([p[0], p[1], p[2], h, w, l, wrap(-ry - math.pi / 2)])
        flags.append(row)
        bbox.append([float(f[4]), float(f[5]), float(f[6]), float(f[7])])
        alpha.append(float(f[3]))
    return {"boxes": np.array(boxes, dtype=np.float64).reshape(-1, 7),
            "flags": np.array(flags, dtype=bool).reshape(-1, len(diffs)).T.copy(),
            "bbox": np.array(bbox, dtype=np.float64).reshape(-1, 4), "alpha": np.array(alpha, dtype=np.float64),
            "dontcare": np.array(dc, dtype=np.float64).reshape(-1, 4)}


def label_line(name, box, calib=MEAN_CALIB, image_hw=IMAGE_HW, trunc=0.0, occ=0, bbox=None, alpha=None, digits=2):
    """the KITTI label line of a lidar box under the frame's calibration; 2D box and alpha are the projection's unless
    given (a box off the image: 0 0 0 0)"""
    p = project_box(box, calib, image_hw)
    row = p["row"]
    bb = row[1:5] if bbox is None else bbox
    al = row[0] if alpha is None else alpha
    x, y, z, h, w, l, r = (float(v) for v in box)
    c = lidar_to_cam(calib) @ np.array([x, y, z, 1.0])
    f = f"{{:.{digits}f}}".format
    return " ".join([name, f(trunc), str(int(occ)), f(al)] + [f(v) for v in bb] + [f(h), f(w), f(l), f(c[0]), f(c[1]), f(c[2]),
                                                                                    f(-r - math.pi / 2)])


def dontcare_line(region):
    return "DontCare -1 -1 -10 " + " ".join(f"{v:.2f}" for v in region) + " -1 -1 -1 -1000 -1000 -1000 -10"


# ---------------------------------------------------------------------------------------------------- matching
def match_frame(iou, scores, ignored, thr, skip, dc_overlap):
    """section 1b's walk (tests/eval_ref.match_frame's rules) with the three additions: a skipped detection (off the
    image, or under the difficulty's height bar) is IGNORED and takes nothing; a detection left FP whose DontCare overlap
    is > 0.5 becomes IGNORED.  Plain loops."""
    n_det, n_gt = iou.shape
    order = sorted(range(n_det), key=lambda d: (-float(scores[d]), d))
    taken = [False] * n_gt
    status, matched = [0] * n_det, [-1] * n_det
    for d in order:
        if skip[d]:
            status[d] = -1
            continue
        best_valid, best_ign = -1, -1
        for g in range(n_gt):
            if taken[g] or not iou[d, g] > thr:
                continue
            if ignored[g]:
                if best_ign < 0 or iou[d, g] > iou[d, best_ign]:
                    best_ign = g
            elif best_valid < 0 or iou[d, g] > iou[d, best_valid]:
                best_valid = g
        if best_valid >= 0:
            status[d], matched[d], taken[best_valid] = 1, best_valid, True
        elif best_ign >= 0:
            status[d], matched[d], taken[best_ign] = -1, best_ign, True
    for d in range(n_det):
        if status[d] == 0 and dc_overlap[d] > 0.5:
            status[d] = -1
    return np.array(status, dtype=np.int64), np.array(matched, dtype=np.int64)


def evaluate_frame(det_boxes, det_scores, gt, calib=MEAN_CALIB, image_hw=IMAGE_HW, diffs=DIFFS, thr=(0.7, 0.7, 0.7),
                   min_height=None):
    """gt: frame_ground_truth's dict.  -> dict: rows (n,12), on (n,), heights, dc_overlap, depths / raw / angles (lists, for
    the guards), iou (3,n,G), status / matched (3,n_diff,n), similarity (n_diff,n)"""
    det = np.asarray(det_boxes, dtype=np.float64).reshape(-1, 7)
    n, G = len(det), len(gt["boxes"])
    proj = [project_box(d, calib, image_hw) for d in det]
    rows = np.array([p["row"] for p in proj], dtype=np.float64).reshape(n, 12)
    on = np.array([p["on"] for p in proj], dtype=bool).reshape(n)
    heights = rows[:, 4] - rows[:, 2]
    dco = np.array([dontcare_overlap(rows[d, 1:5], gt["dontcare"]) if on[d] else 0.0 for d in range(n)]).reshape(n)
    iou = np.zeros((3, n, G), dtype=np.float64)
    for i in range(n):
        for j in range(G):
            iou[0, i, j], iou[1, i, j] = R.iou_pair(det[i], gt["boxes"][j])
            iou[2, i, j] = iou_2d(rows[i, 1:5], gt["bbox"][j])
    bars = [MIN_HEIGHT[d] for d in diffs] if min_height is None else list(min_height)
    status = np.zeros((3, len(diffs), n), dtype=np.int64)
    matched = np.zeros((3, len(diffs), n), dtype=np.int64)
    sim = np.zeros((len(diffs), n), dtype=np.float64)
    for k in range(len(diffs)):
        skip = [(not on[d]) or (bars[k] is not None and heights[d] < bars[k]) for d in range(n)]
        for m in range(3):
            status[m, k], matched[m, k] = match_frame(iou[m], det_scores, gt["flags"][k], thr[m], skip, dco)
        for d in range(n):
            if status[2, k, d] == 1:
                sim[k, d] = (1 + math.cos(rows[d, 0] - gt["alpha"][matched[2, k, d]])) / 2
    return {"rows": rows, "on": on, "heights": heights, "dc_overlap": dco, "iou": iou, "status": status, "matched": matched,
            "similarity": sim, "depths": [p["depths"] for p in proj], "raw": [p["raw"] for p in proj],
            "angles": [p["angles"] for p in proj]}


# ---------------------------------------------------------------------------------------------------- AP, AOS
def ap_and_aos(scores, status, similarity, n_valid_gt, recall_points=40):
    """pooled (score, status, similarity) of the bbox matching in (frame, index) order -> (AP, AOS): IGNORED dropped,
    stable sort by descending score, p = tp / (tp + fp), s = sum(similarity) / (tp + fp); at every recall point the largest
    p (and, separately, the largest s) at a recall >= it; NaN without a valid ground truth"""
    if n_valid_gt == 0:
        return float("nan"), float("nan")
    rows = [(float(s), int(t), float(v)) for s, t, v in zip(scores, status, similarity) if int(t) != -1]
    rows.sort(key=lambda p: -p[0])
    tp = n = 0
    acc = 0.0
    curve = []
    for _, t, v in rows:
        n += 1
        tp += 1 if t == 1 else 0
        acc += v
        curve.append((tp / n_valid_gt, tp / n, acc / n))
    rs = [k / 40 for k in range(1, 41)] if recall_points == 40 else [k / 10 for k in range(0, 11)]
    ap = sum(max([p for rec, p, _ in curve if rec >= r], default=0.0) for r in rs) / len(rs)
    aos = sum(max([s for rec, _, s in curve if rec >= r], default=0.0) for r in rs) / len(rs)
    return ap, aos


class RefEvaluator:
    """frame-by-frame accumulation with the functions above"""

    def __init__(self, cls_name="Car", diffs=DIFFS, thr=None, recall_points=40):
        t = THRES[cls_name] if thr is None else thr
        self.cls_name, self.diffs, self.recall_points = cls_name, tuple(diffs), recall_points
        self.thr = (t, t, t) if np.isscalar(t) else tuple(t)
        self.scores = []
        self.status = {m: [[] for _ in self.diffs] for m in METRICS}
        self.sim = [[] for _ in self.diffs]
        self.n_gt = [0] * len(self.diffs)
        self.n_ignored = [0] * len(self.diffs)
        self.frames = []

    def add_frame(self, det_boxes, det_scores, lines, calib=None, image_hw=IMAGE_HW):
        calib = MEAN_CALIB if calib is None else calib
        gt = frame_ground_truth(lines, self.cls_name, self.diffs, calib)
        r = evaluate_frame(det_boxes, det_scores, gt, calib, image_hw, self.diffs, self.thr)
        self.scores += [float(s) for s in det_scores]
        for k in range(len(self.diffs)):
            for m, metric in enumerate(METRICS):
                self.status[metric][k] += [int(v) for v in r["status"][m][k]]
            self.sim[k] += [float(v) for v in r["similarity"][k]]
            self.n_gt[k] += int((~gt["flags"][k]).sum())
            self.n_ignored[k] += int(((r["status"][2][k] == -1) & (r["matched"][2][k] < 0)).sum())
        r["gt"] = gt
        self.frames.append(r)
        return r

    def compute(self):
        out = {"n_gt": {d: self.n_gt[k] for k, d in enumerate(self.diffs)}, "n_det": len(self.scores),
               "n_ignored": {d: self.n_ignored[k] for k, d in enumerate(self.diffs)}, "aos": {}}
        zeros = [0.0] * len(self.scores)
        for metric in METRICS:
            out[metric] = {d: ap_and_aos(self.scores, self.status[metric][k], zeros, self.n_gt[k], self.recall_points)[0]
                           for k, d in enumerate(self.diffs)}
        for k, d in enumerate(self.diffs):
            out["aos"][d] = ap_and_aos(self.scores, self.status["bbox"][k], self.sim[k], self.n_gt[k], self.recall_points)[1]
        return out


def result_line(cls_name, row, score):
    return cls_name + " -1 -1 " + " ".join("%.2f" % v for v in row) + " %.4f" % score


# ---------------------------------------------------------------------------------------------- scene generator
def perturbed_calib(rng):
    """the mean calibration perturbed: a few degrees, a few centimetres, focal length +- 5 %"""
    ax, ay, az = rng.uniform(-0.05, 0.05, 3)          # radians: up to ~3 degrees
    cx, sx, cy, sy, cz, sz = math.cos(ax), math.sin(ax), math.cos(ay), math.sin(ay), math.cos(az), math.sin(az)
    rot = (np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
           @ np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]))
    Tr = MEAN_TR.copy()
    Tr[:3, :3] = rot @ MEAN_TR[:3, :3]
    Tr[:3, 3] = MEAN_TR[:3, 3] + rng.uniform(-0.05, 0.05, 3)
    P2 = MEAN_P2.copy()
    f = rng.uniform(0.95, 1.05)
    P2[0, 0] *= f
    P2[1, 1] *= f
    P2[0, 2] += rng.uniform(-8, 8)
    P2[1, 2] += rng.uniform(-5, 5)
    return P2, Tr, MEAN_R0.copy()


def make_frame(rng, top_k=20, cls_name="Car"):
    """-> dict: det (n,7) float32, scores (n,) float32 distinct, lines, calib, image_hw.  Ground truths in front of the
    camera at 5..65 m (most on the image, some beside it; far ones under the height bars), detections = ground truths jittered so
    that the IoUs of all three metrics fall on both sides of 0.5 / 0.7, anchor-sized clutter, a Van and other classes'
    lines, 0..5 DontCare regions — some drawn around a clutter detection's 2D box."""
    calib = perturbed_calib(rng)
    hw = (int(rng.choice([370, 375, 376])), int(rng.choice([1224, 1242, 1238])))
    gts = []
    for _ in range(int(rng.integers(0, 11))):
        x = rng.uniform(5, 65)
        gts.append([x, rng.uniform(-0.95, 0.95) * x, rng.uniform(-2, -1.2), rng.uniform(1.4, 1.8), rng.uniform(1.5, 1.8),
                    rng.uniform(3.4, 4.5), rng.uniform(-math.pi, math.pi)])
    lines = []
    for g in gts:
        name = "Van" if rng.random() < 0.12 else cls_name
        lines.append(label_line(name, g, calib, hw, trunc=float(rng.choice([0.0, 0.1, 0.25, 0.4])), occ=int(rng.integers(0, 3)),
                                digits=6))
    dets = []
    for g in gts:
        for _ in range(int(rng.choice([0, 1, 2], p=[0.2, 0.6, 0.2]))):
            d = np.array(g)
            d[0:2] += rng.normal(0, 0.25, 2)
            d[2] += rng.normal(0, 0.1)
            d[6] += rng.normal(0, 0.1) + (math.pi if rng.random() < 0.2 else 0.0)          # some headings flipped: AOS < AP
            d[3:6] *= rng.uniform(0.93, 1.07, 3)
            dets.append(d)
    for _ in range(int(rng.integers(1, 6))):          # clutter of anchor size
        x = rng.uniform(0.5, 68)          # (the nearest ones have corners behind the camera)
        dets.append(np.array([x, rng.uniform(-1.1, 1.1) * x, -1.78, 1.56, 1.6, 3.9, rng.choice([0.0, 1.5])]))          # (not pi/2: -r - pi/2 would sit on the wrap seam)
    dets = [dets[i] for i in rng.permutation(len(dets))][:top_k]
    det = np.array(dets, dtype=np.float64).reshape(-1, 7).astype(np.float32)
    n = det.shape[0]
    ticks = rng.choice(40000, size=n, replace=False)
    scores = (np.float32(0.96) + ticks.astype(np.float32) * np.float32(2.0 ** -20)).astype(np.float32)
    for _ in range(int(rng.integers(0, 6))):
        d = det[int(rng.integers(0, n))].astype(np.float64)
        p = project_box(d, calib, hw)
        if p["on"] and rng.random() < 0.7:          # around a detection's 2D box, grown or shifted
            x1, y1, x2, y2 = p["row"][1:5]
            sh = rng.uniform(-0.7, 0.7) * (x2 - x1)
            region = [x1 - 5 + sh, y1 - 5, x2 + 5 + sh, y2 + 5]
        else:
            x1, y1 = rng.uniform(0, 1000), rng.uniform(100, 250)
            region = [x1, y1, x1 + rng.uniform(20, 200), y1 + rng.uniform(10, 60)]
        lines.insert(int(rng.integers(0, len(lines) + 1)), dontcare_line(region))
    for name in ("Pedestrian", "Cyclist", "Tram", "Misc"):
        if rng.random() < 0.3 and n:
            lines.insert(int(rng.integers(0, len(lines) + 1)),
                         label_line(name, det[int(rng.integers(0, n))].astype(np.float64), calib, hw, digits=6))
    return {"det": det, "scores": scores, "lines": lines, "calib": calib, "image_hw": hw}


def make_scene(seed, n_frames=8, top_k=20, cls_name="Car"):
    rng = np.random.default_rng(seed)
    return [make_frame(rng, top_k, cls_name) for _ in range(n_frames)]
