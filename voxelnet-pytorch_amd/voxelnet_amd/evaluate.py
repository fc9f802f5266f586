"""Detection scoring — the stage the reference leaves empty (voxelnet/eval.py:4-5 is a stub; protocol: DESIGN.md §1b):
KITTI-style average precision in the bird's-eye view and in 3D, with the per-pair and per-frame work on the device.

  device (csrc/eval.hip): `vn_box_iou_rotated` — the IoU of two ROTATED boxes, float64; `vn_eval_match` — one
         workgroup per frame fills the frame's BEV and 3D IoU tables and runs the greedy matching of the decoded
         detections (BoxDecoder.decode_device: they never leave HBM) against the frame's ground truths for both metrics
         and every difficulty, in one launch per batch
  host   (this module): label lines -> ground-truth boxes + per-difficulty flags (O(boxes)); one status byte and one
         score per detection, copied back asynchronously and read at `compute()`; the precision / recall arithmetic.

There is no CPU path for the IoU or the matching: CPU tensors raise VoxelnetHipError.

Stated divergences from KITTI's official tool: the greedy pass is detection-ordered (PASCAL style), not
KITTI's per-ground-truth pass; DontCare regions and the 2D-height filter on detections need the image projection and are
not applied; the calibration is the mean calibration of targets.py.

`KittiDetectionEvaluator` closes the last two: it projects every detection into the image with the
frame's own calibration (`vn_boxes_to_image`), scores the 2D `bbox` metric and the orientation score AOS beside `bev` and
`3d`, applies DontCare regions and the 2D-height bar (`vn_eval_match_image`), and writes KITTI result lines — the form
KITTI's devkit and the test server take."""
import math
import os

import numpy as np
import torch

from . import _lib
from .targets import _R_RECT_0, _T_VELO_2_CAM, CLASS_CFG, MAX_GT, label_to_gt_box_3d

# difficulty -> (minimum 2D box height y2 - y1, maximum occlusion, maximum truncation); None: no filter.  "all" exists
# because targets.lidar_box_to_label_line's synthetic lines carry zeros in those fields.
DIFFICULTIES = {"all": None, "easy": (40.0, 0.0, 0.15), "moderate": (25.0, 1.0, 0.30), "hard": (25.0, 2.0, 0.50)}
IOU_THRES = {"Car": 0.7, "Pedestrian": 0.5, "Cyclist": 0.5}
METRICS = ("bev", "3d")          # axis 1 of vn_eval_match's outputs: VN_EVAL_BEV, VN_EVAL_3D
TP, FP, IGNORED, EMPTY = 1, 0, -1, -2


def _need_f64_boxes(t, what):
    if not (torch.is_tensor(t) and t.is_cuda):
        raise _lib.VoxelnetHipError(f"{what} must be a HIP tensor (there is no CPU path)")
    if t.dim() != 2 or t.shape[1] != 7:
        raise ValueError(f"{what}: (n,7) boxes (x,y,z,h,w,l,r) expected, got {tuple(t.shape)}")
    return t.detach().to(torch.float64).contiguous()


def box_iou_rotated(a, b, metric="bev"):
    """a (na,7), b (nb,7) HIP tensors of boxes (x,y,z,h,w,l,r) -> (na,nb) float64 HIP tensor of rotated IoUs, metric
    'bev' or '3d', enqueued on the current stream (float32 inputs are widened exactly)."""
    if metric not in METRICS:
        raise ValueError(f"metric {metric!r}: 'bev' or '3d'")
    a, b = _need_f64_boxes(a, "a"), _need_f64_boxes(b, "b")
    if a.device != b.device:
        raise ValueError("a and b live on different devices")
    out = torch.empty((a.shape[0], b.shape[0]), dtype=torch.float64, device=a.device)
    with _lib.on_device(a.device):
        _lib.call("vn_box_iou_rotated", a.data_ptr(), a.shape[0], b.data_ptr(), b.shape[0], METRICS.index(metric), out.data_ptr(),
                  _lib.raw_stream())
    return out


def gt_flags_from_labels(labels, cls_name="Car", difficulties=("all", "easy", "moderate", "hard")):
    """labels: per frame, the KITTI label lines (`type trunc occ alpha x1 y1 x2 y2 h w l x y z ry`).
    -> (boxes: per frame (G,7) float64 lidar boxes through label_to_gt_box_3d's conversion, flags: per frame
    (n_diff,G) uint8 — 0 valid, 1 ignored —, n_valid: (n_frames, n_diff) int64 count of the valid ones).
    A line of class `cls_name` is a candidate, ignored at a difficulty whose filter it fails; a line of another class in
    CLASS_CFG[cls_name]['accept'] (Van for Car) is ignored at every difficulty; every other line is dropped."""
    accept = CLASS_CFG[cls_name]["accept"]
    filters = [DIFFICULTIES[d] for d in difficulties]
    boxes, flags = [], []
    n_valid = np.zeros((len(labels), len(filters)), dtype=np.int64)
    for i, label in enumerate(labels):
        kept, fl = [], []
        for line in label:
            f = line.split()
            if f[0] != cls_name and f[0] not in accept:
                continue
            kept.append(line)
            if f[0] != cls_name:
                fl.append([1] * len(filters))
                continue
            trunc, occ, height = float(f[1]), float(f[2]), float(f[7]) - float(f[5])
            fl.append([0 if flt is None or (height >= flt[0] and occ <= flt[1] and trunc <= flt[2]) else 1 for flt in filters])
        boxes.append(label_to_gt_box_3d([kept], "", "lidar")[0])          # ("": every line handed over is converted)
        fa = np.array(fl, dtype=np.uint8).reshape(-1, len(filters)).T
        flags.append(np.ascontiguousarray(fa))
        n_valid[i] = (fa == 0).sum(axis=1)
    return boxes, flags, n_valid


def average_precision(scores, status, n_valid_gt, recall_points=40):
    """scores, status: the pooled detections in (frame, index) order, status TP / FP / IGNORED.  IGNORED ones are dropped,
    the rest sorted by descending score (stable); precision = tp/(tp+fp), recall = tp/n_valid_gt cumulatively;
    p_interp(r) = the largest precision at a recall >= r (0 when that recall is never reached); AP = mean of p_interp
    over r = 1/40 ... 40/40 (recall_points = 40) or 0, 0.1 ... 1 (11).  n_valid_gt == 0 -> NaN.  Float64."""
    if recall_points not in (40, 11):
        raise ValueError("recall_points: 40 (R40) or 11 (R11)")
    n_valid_gt = int(n_valid_gt)
    if n_valid_gt == 0:
        return float("nan")
    scores, status = np.asarray(scores, dtype=np.float64), np.asarray(status, dtype=np.int64)
    keep = status != IGNORED
    scores, status = scores[keep], status[keep]
    order = np.argsort(-scores, kind="stable")
    tp = np.cumsum(status[order] == TP)
    precision = tp / np.arange(1, tp.size + 1, dtype=np.float64)
    # best precision from position i to the end: the recall only grows along the list
    best = np.maximum.accumulate(precision[::-1])[::-1] if tp.size else precision
    den, ks = (40, range(1, 41)) if recall_points == 40 else (10, range(0, 11))
    total = 0.0
    for k in ks:
        # first position whose recall tp/n_valid_gt >= k/den, in integers
        i = int(np.searchsorted(tp * den, k * n_valid_gt, side="left"))
        total += float(best[i]) if i < tp.size else 0.0
    return total / len(ks)


class DetectionEvaluator:
    """Accumulates detections over an evaluation pass and turns them into AP.

    update(boxes, scores, counts, labels): one batch.  boxes (B,top_k,7) f32, scores (B,top_k) f32, counts (B,) int32
      HIP tensors as BoxDecoder.decode_device returns them — or the lists of NumPy arrays BoxDecoder.__call__ returns
      (counts = None), which are uploaded; labels: the batch's label lines.  One vn_eval_match launch; the status bytes
      and the scores are copied back asynchronously and not waited for.
    compute() -> {"bev": {difficulty: AP}, "3d": {difficulty: AP}, "n_gt": {difficulty: n}, "n_det": n}
    reset()"""

    def __init__(self, cls_name="Car", device="cuda:0", iou_thres=None, difficulties=("all", "easy", "moderate", "hard"),
                 top_k=20, recall_points=40):
        self.cls_name = cls_name
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.VoxelnetHipError("DetectionEvaluator needs a HIP device (no CPU path)")
        thr = IOU_THRES[cls_name] if iou_thres is None else iou_thres
        self.iou_thres = (float(thr), float(thr)) if np.isscalar(thr) else (float(thr[0]), float(thr[1]))      # (bev, 3d)
        self.difficulties = tuple(difficulties)
        if not 1 <= len(self.difficulties) <= _lib.VN_EVAL_MAX_DIFF or any(d not in DIFFICULTIES for d in self.difficulties):
            raise ValueError(f"difficulties: 1..{_lib.VN_EVAL_MAX_DIFF} of {sorted(DIFFICULTIES)}")
        if not 1 <= int(top_k) <= _lib.VN_EVAL_MAX_TOPK:
            raise ValueError(f"top_k: 1..{_lib.VN_EVAL_MAX_TOPK}")
        if recall_points not in (40, 11):
            raise ValueError("recall_points: 40 (R40) or 11 (R11)")
        self.top_k, self.recall_points = int(top_k), recall_points
        self.reset()

    def reset(self):
        self._pending = []          # (status host, scores host, event, tensors the queued work uses)
        self._n_valid = np.zeros(len(self.difficulties), dtype=np.int64)

    def _upload(self, array):
        return torch.from_numpy(array).pin_memory().to(self.device, non_blocking=True)

    def _detections(self, boxes, scores, counts):
        if torch.is_tensor(boxes) or torch.is_tensor(scores) or torch.is_tensor(counts):
            if not all(torch.is_tensor(t) and t.is_cuda for t in (boxes, scores, counts)):
                raise _lib.VoxelnetHipError("update: boxes / scores / counts must be HIP tensors (there is no CPU path)")
            if boxes.dim() != 3 or boxes.shape[2] != 7 or tuple(scores.shape) != tuple(boxes.shape[:2]) or \
                    tuple(counts.shape) != (boxes.shape[0],):
                raise ValueError("update: boxes (B,top_k,7), scores (B,top_k), counts (B,) expected")
            return (boxes.detach().float().contiguous(), scores.detach().float().contiguous(),
                    counts.detach().to(torch.int32).contiguous())
        # the list-of-NumPy form of BoxDecoder.__call__
        B = len(boxes)
        bh = np.zeros((B, self.top_k, 7), dtype=np.float32)
        sh = np.zeros((B, self.top_k), dtype=np.float32)
        ch = np.zeros(B, dtype=np.int32)
        for b in range(B):
            n = len(scores[b])
            if n > self.top_k:
                raise ValueError(f"{n} detections in one frame; this evaluator was built for top_k = {self.top_k}")
            bh[b, :n] = np.asarray(boxes[b], dtype=np.float32).reshape(n, 7)
            sh[b, :n] = scores[b]
            ch[b] = n
        return self._upload(bh), self._upload(sh), self._upload(ch)

    def update(self, boxes, scores, counts, labels):
        with _lib.on_device(self.device):
            boxes, scores, counts = self._detections(boxes, scores, counts)
            B, top_k = int(boxes.shape[0]), int(boxes.shape[1])
            if len(labels) != B:
                raise ValueError(f"{len(labels)} labels for {B} frames")
            if B == 0:
                return
            if top_k > _lib.VN_EVAL_MAX_TOPK:
                raise _lib.VoxelnetHipError(f"top_k = {top_k}; vn_eval_match takes at most {_lib.VN_EVAL_MAX_TOPK}")
            gt_boxes, gt_flags, n_valid = gt_flags_from_labels(labels, self.cls_name, self.difficulties)
            n_diff = len(self.difficulties)
            G = max([g.shape[0] for g in gt_boxes] + [1])
            if G > MAX_GT:
                raise _lib.VoxelnetHipError(f"{G} ground-truth boxes in one frame; vn_eval_match takes at most {MAX_GT}")
            gt = np.zeros((B, G, 7), dtype=np.float64)
            fl = np.zeros((B, n_diff, G), dtype=np.uint8)
            gc = np.zeros(B, dtype=np.int32)
            for b in range(B):
                n = gt_boxes[b].shape[0]
                gc[b] = n
                gt[b, :n] = gt_boxes[b]
                fl[b, :, :n] = gt_flags[b]
            gt_d, fl_d, gc_d = self._upload(gt), self._upload(fl), self._upload(gc)
            dev = self.device
            status = torch.empty((B, 2, n_diff, top_k), dtype=torch.int8, device=dev)
            matched = torch.empty((B, 2, n_diff, top_k), dtype=torch.int32, device=dev)
            nbytes = _lib.load().vn_eval_match_workspace_bytes(B, top_k, G)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            _lib.call("vn_eval_match", boxes.data_ptr(), scores.data_ptr(), counts.data_ptr(), gt_d.data_ptr(), gc_d.data_ptr(),
                      fl_d.data_ptr(), B, top_k, G, n_diff, self.iou_thres[0], self.iou_thres[1], status.data_ptr(),
                      matched.data_ptr(), None, ws.data_ptr(), nbytes, _lib.raw_stream())
            # queued, not waited for: compute() synchronises on the event
            status_h = torch.empty(status.shape, dtype=torch.int8).pin_memory()
            scores_h = torch.empty(scores.shape, dtype=torch.float32).pin_memory()
            status_h.copy_(status, non_blocking=True)
            scores_h.copy_(scores, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            self._pending.append((status_h, scores_h, ev, (boxes, scores, counts, gt_d, fl_d, gc_d, status, matched, ws)))
            self._n_valid += n_valid.sum(axis=0)

    def compute(self):
        n_diff = len(self.difficulties)
        scores = [np.zeros(0, dtype=np.float32)]
        status = [[[np.zeros(0, dtype=np.int8)] for _ in range(n_diff)] for _ in METRICS]
        for i, (status_h, scores_h, ev, _) in enumerate(self._pending):
            ev.synchronize()
            self._pending[i] = (status_h, scores_h, ev, ())          # the device side of this batch is done
            st, sc = status_h.numpy(), scores_h.numpy()          # (B, 2, n_diff, top_k), (B, top_k)
            there = st[:, 0, 0, :] != EMPTY                      # the slots below the frame's count: same for every matching
            scores.append(sc[there])                             # (boolean indexing keeps the (frame, index) order)
            for m in range(len(METRICS)):
                for k in range(n_diff):
                    status[m][k].append(st[:, m, k, :][there])
        sc = np.concatenate(scores)
        out = {"n_gt": {d: int(self._n_valid[k]) for k, d in enumerate(self.difficulties)}, "n_det": int(sc.size)}
        for m, metric in enumerate(METRICS):
            out[metric] = {d: average_precision(sc, np.concatenate(status[m][k]), self._n_valid[k], self.recall_points)
                           for k, d in enumerate(self.difficulties)}
        return out


# ------------------------------------------------------------------------------ image-plane scoring
KITTI_METRICS = ("bev", "3d", "bbox")          # axis 1 of vn_eval_match_image's outputs: VN_EVAL_BEV, VN_EVAL_3D, VN_EVAL_BBOX
# KITTI's protocol: a line of a neighbour class is ignored at every difficulty.  (Not CLASS_CFG's `accept`, which training reads.)
NEIGHBOUR_CLASSES = {"Car": ("Van",), "Pedestrian": ("Person_sitting",), "Cyclist": ()}
# difficulty -> the 2D height under which a DETECTION is ignored (the ground-truth filter's bar; none for "all")
MIN_HEIGHT = {"all": 0.0, "easy": 40.0, "moderate": 25.0, "hard": 25.0}
IMAGE_SHAPE = (375, 1242)          # (H, W), as DeviceCollate
# the mean P2 (voxelnet/config.py:102-127): the float32 values the FOV crop is tested with (tests/golden/fov_crop.npz, `P`)
MEAN_P2 = np.array([[719.787109375, 0.0, 608.4630126953125, 44.95387649536133],
                    [0.0, 719.787109375, 174.54510498046875, 0.10668549686670303],
                    [0.0, 0.0, 1.0, 0.00301064713858068]], dtype=np.float64)


def mean_calib():
    """-> (P2 (3,4), Tr_velo_to_cam (4,4), R0_rect (4,4)) float64: the mean calibration (targets.py's matrices)"""
    return MEAN_P2.copy(), _T_VELO_2_CAM.astype(np.float64), _R_RECT_0.astype(np.float64)


def load_kitti_calib(path):
    """KITTI object calibration file -> (P2 (3,4), Tr_velo_to_cam (4,4), R0_rect (4,4)) float64, found by their keys"""
    rows = {}
    with open(path) as fh:
        for line in fh:
            if ":" in line:
                key, val = line.split(":", 1)
                rows[key.strip()] = np.array(val.split(), dtype=np.float64)
    P2 = rows["P2"].reshape(3, 4)
    Tr, R0 = np.eye(4), np.eye(4)
    Tr[:3] = rows["Tr_velo_to_cam"].reshape(3, 4)
    R0[:3, :3] = rows["R0_rect"].reshape(3, 3)
    return P2, Tr, R0


def _wrap(a):
    """into (-pi, pi]"""
    return a - 2.0 * math.pi * math.ceil((a - math.pi) / (2.0 * math.pi))


def _calib_rows(calib):
    """(P2, Tr, R0) or None -> (the kernel's 24 doubles [M | P2], R0.Tr (4,4))"""
    P2, Tr, R0 = (np.asarray(m, dtype=np.float64) for m in (mean_calib() if calib is None else calib))
    if P2.shape != (3, 4) or Tr.shape != (4, 4) or R0.shape != (4, 4):
        raise ValueError("calibration: P2 (3,4), Tr_velo_to_cam (4,4), R0_rect (4,4)")
    full = R0 @ Tr
    return np.concatenate([full[:3].reshape(-1), P2.reshape(-1)]), full


def kitti_ground_truth(labels, cls_name="Car", difficulties=("all", "easy", "moderate", "hard"), calibs=None):
    """KITTI's protocol for the ground truths.  labels: per frame, the label lines; calibs: per frame (P2, Tr, R0) or None
    (the mean calibration).  -> per frame: boxes (G,7) float64 lidar (centre through inv(R0.Tr) of the FRAME,
    r = wrap(-ry - pi/2), no 5-degree snap), flags (n_diff,G) uint8 (0 valid, 1 ignored), bbox (G,4) and alpha (G,) as
    written in the label, dontcare (D,4); and n_valid (n_frames, n_diff).  A line of the class is a candidate, ignored
    where it fails the difficulty's filter; a line of a neighbour class (NEIGHBOUR_CLASSES) is ignored everywhere;
    DontCare lines give 2D regions only; every other line is dropped."""
    neighbours = NEIGHBOUR_CLASSES[cls_name]
    filters = [DIFFICULTIES[d] for d in difficulties]
    out = {"boxes": [], "flags": [], "bbox": [], "alpha": [], "dontcare": []}
    n_valid = np.zeros((len(labels), len(filters)), dtype=np.int64)
    for i, label in enumerate(labels):
        inv = np.linalg.inv(_calib_rows(None if calibs is None else calibs[i])[1])
        boxes, fl, bbox, alpha, dc = [], [], [], [], []
        for line in label:
            f = line.split()
            if f[0] == "DontCare":
                dc.append([float(v) for v in f[4:8]])
                continue
            if f[0] != cls_name and f[0] not in neighbours:
                continue
            if f[0] != cls_name:
                fl.append([1] * len(filters))
            else:
                trunc, occ, height = float(f[1]), float(f[2]), float(f[7]) - float(f[5])
                fl.append([0 if flt is None or (height >= flt[0] and occ <= flt[1] and trunc <= flt[2]) else 1 for flt in filters])
            h, w, l, x, y, z, ry = (float(v) for v in f[8:15])
            p = inv @ np.array([x, y, z, 1.0])
            boxes.append([p[0], p[1], p[2], h, w, l, _wrap(-ry - math.pi / 2)])
            bbox.append([float(v) for v in f[4:8]])
            alpha.append(float(f[3]))
        fa = np.ascontiguousarray(np.array(fl, dtype=np.uint8).reshape(-1, len(filters)).T)
        out["boxes"].append(np.array(boxes, dtype=np.float64).reshape(-1, 7))
        out["flags"].append(fa)
        out["bbox"].append(np.array(bbox, dtype=np.float64).reshape(-1, 4))
        out["alpha"].append(np.array(alpha, dtype=np.float64))
        out["dontcare"].append(np.array(dc, dtype=np.float64).reshape(-1, 4))
        n_valid[i] = (fa == 0).sum(axis=1)
    return out, n_valid


def average_orientation_similarity(scores, status, similarity, n_valid_gt, recall_points=40):
    """AOS: average_precision's arithmetic on the `bbox` matching with one difference — the curve is
    cumsum(similarity) / (tp + fp) instead of tp / (tp + fp).  Same drop of IGNORED, same stable sort, same
    best-from-the-right interpolation, same recall points; similarity <= 1 per TP and 0 otherwise, so AOS <= AP."""
    if recall_points not in (40, 11):
        raise ValueError("recall_points: 40 (R40) or 11 (R11)")
    n_valid_gt = int(n_valid_gt)
    if n_valid_gt == 0:
        return float("nan")
    scores, status = np.asarray(scores, dtype=np.float64), np.asarray(status, dtype=np.int64)
    similarity = np.asarray(similarity, dtype=np.float64)
    keep = status != IGNORED
    scores, status, similarity = scores[keep], status[keep], similarity[keep]
    order = np.argsort(-scores, kind="stable")
    tp = np.cumsum(status[order] == TP)
    curve = np.cumsum(similarity[order]) / np.arange(1, tp.size + 1, dtype=np.float64)
    best = np.maximum.accumulate(curve[::-1])[::-1] if tp.size else curve
    den, ks = (40, range(1, 41)) if recall_points == 40 else (10, range(0, 11))
    total = 0.0
    for k in ks:
        i = int(np.searchsorted(tp * den, k * n_valid_gt, side="left"))
        total += float(best[i]) if i < tp.size else 0.0
    return total / len(ks)


def format_result_line(cls_name, row, score):
    """one KITTI result line: `type -1 -1 alpha x1 y1 x2 y2 h w l x y z ry score` (twelve fields with two decimals,
    the score with four); row: vn_boxes_to_image's twelve fields"""
    return f"{cls_name} -1 -1 " + " ".join(f"{float(v):.2f}" for v in row) + f" {float(score):.4f}"


class KittiDetectionEvaluator(DetectionEvaluator):
    """DetectionEvaluator by KITTI's image-plane rules: per-frame calibration, the 2D `bbox` metric,
    AOS, DontCare regions and the 2D-height bar on detections, KITTI result lines.

    update(boxes, scores, counts, labels, calibs=None, image_shapes=None, tags=None): detections as DetectionEvaluator
      takes them; calibs: per frame (P2, Tr_velo_to_cam, R0_rect) or None = the mean calibration (a list may hold None
      too); image_shapes: per frame (H, W), default IMAGE_SHAPE; tags: per frame the name write_results gives its file
      (default: the frame's running number, six digits).  Two launches (vn_boxes_to_image, vn_eval_match_image), then
      queued, unwaited copies.
    compute() -> {"bbox","bev","3d","aos": {difficulty: value}, "n_gt": {difficulty: n}, "n_det": n, "n_ignored":
      {difficulty: detections of the `bbox` matching that are IGNORED without having taken a ground truth: off the image,
      under the height bar, or in a DontCare region}}
    result_lines() -> (tags, per frame the result lines of its on-image detections in score order)
    write_results(directory): one <tag>.txt per frame (an empty file for a frame without detections)."""

    def __init__(self, cls_name="Car", device="cuda:0", iou_thres=None, difficulties=("all", "easy", "moderate", "hard"),
                 top_k=20, recall_points=40):
        super().__init__(cls_name, device, iou_thres, difficulties, top_k, recall_points)
        thr = IOU_THRES[cls_name] if iou_thres is None else iou_thres
        self.iou_thres = (float(thr),) * 3 if np.isscalar(thr) else tuple(float(t) for t in thr)      # (bev, 3d, bbox)
        if len(self.iou_thres) != 3:
            raise ValueError("iou_thres: one number or (bev, 3d, bbox)")

    def reset(self):
        super().reset()
        self._tags = []

    def update(self, boxes, scores, counts, labels, calibs=None, image_shapes=None, tags=None):
        with _lib.on_device(self.device):
            boxes, scores, counts = self._detections(boxes, scores, counts)
            B, top_k = int(boxes.shape[0]), int(boxes.shape[1])
            if len(labels) != B or any(v is not None and len(v) != B for v in (calibs, image_shapes, tags)):
                raise ValueError(f"labels / calibs / image_shapes / tags: one per frame ({B}) expected")
            if B == 0:
                return
            if top_k > _lib.VN_EVAL_MAX_TOPK:
                raise _lib.VoxelnetHipError(f"top_k = {top_k}; vn_eval_match_image takes at most {_lib.VN_EVAL_MAX_TOPK}")
            gts, n_valid = kitti_ground_truth(labels, self.cls_name, self.difficulties, calibs)
            n_diff = len(self.difficulties)
            G = max([g.shape[0] for g in gts["boxes"]] + [1])
            D = max(d.shape[0] for d in gts["dontcare"])
            if G > MAX_GT:
                raise _lib.VoxelnetHipError(f"{G} ground-truth boxes in one frame; vn_eval_match_image takes at most {MAX_GT}")
            if D > _lib.VN_EVAL_MAX_DC:
                raise _lib.VoxelnetHipError(f"{D} DontCare regions in one frame; vn_eval_match_image takes at most {_lib.VN_EVAL_MAX_DC}")
            gt = np.zeros((B, G, 7), dtype=np.float64)
            fl = np.zeros((B, n_diff, G), dtype=np.uint8)
            gc = np.zeros(B, dtype=np.int32)
            gb = np.zeros((B, G, 4), dtype=np.float64)
            ga = np.zeros((B, G), dtype=np.float64)
            dcb = np.zeros((B, max(D, 1), 4), dtype=np.float64)
            dcc = np.zeros(B, dtype=np.int32)
            cal = np.zeros((B, 24), dtype=np.float64)
            hw = np.zeros((B, 2), dtype=np.int32)
            for b in range(B):
                n, nd = gts["boxes"][b].shape[0], gts["dontcare"][b].shape[0]
                gc[b], dcc[b] = n, nd
                gt[b, :n], fl[b, :, :n], gb[b, :n], ga[b, :n] = gts["boxes"][b], gts["flags"][b], gts["bbox"][b], gts["alpha"][b]
                dcb[b, :nd] = gts["dontcare"][b]
                cal[b] = _calib_rows(None if calibs is None else calibs[b])[0]
                hw[b] = IMAGE_SHAPE if image_shapes is None or image_shapes[b] is None else tuple(int(v) for v in image_shapes[b])[:2]
            mh = np.array([MIN_HEIGHT[d] for d in self.difficulties], dtype=np.float64)
            host = (gt, gc, fl, gb, ga, dcb, dcc, cal, hw, mh)
            gt_d, gc_d, fl_d, gb_d, ga_d, dcb_d, dcc_d, cal_d, hw_d, mh_d = (self._upload(a) for a in host)
            dev = self.device
            rows = torch.empty((B, top_k, _lib.VN_EVAL_IMAGE_ROW), dtype=torch.float64, device=dev)
            on = torch.empty((B, top_k), dtype=torch.uint8, device=dev)
            status = torch.empty((B, 3, n_diff, top_k), dtype=torch.int8, device=dev)
            matched = torch.empty((B, 3, n_diff, top_k), dtype=torch.int32, device=dev)
            sim = torch.empty((B, n_diff, top_k), dtype=torch.float64, device=dev)
            nbytes = _lib.load().vn_eval_match_workspace_bytes(B, top_k, G)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            stream = _lib.raw_stream()
            _lib.call("vn_boxes_to_image", boxes.data_ptr(), counts.data_ptr(), cal_d.data_ptr(), hw_d.data_ptr(), B, top_k,
                      rows.data_ptr(), on.data_ptr(), stream)
            _lib.call("vn_eval_match_image", boxes.data_ptr(), scores.data_ptr(), counts.data_ptr(), gt_d.data_ptr(), gc_d.data_ptr(),
                      fl_d.data_ptr(), rows.data_ptr(), on.data_ptr(), gb_d.data_ptr(), ga_d.data_ptr(), dcb_d.data_ptr(),
                      dcc_d.data_ptr(), mh_d.data_ptr(), B, top_k, G, D, n_diff, self.iou_thres[0], self.iou_thres[1],
                      self.iou_thres[2], status.data_ptr(), matched.data_ptr(), sim.data_ptr(), None, ws.data_ptr(), nbytes, stream)
            # queued, not waited for: compute() / result_lines() synchronise on the event
            dev_t = (status, matched, sim, rows, on, scores)
            host_t = tuple(torch.empty(t.shape, dtype=t.dtype).pin_memory() for t in dev_t)
            for h, d in zip(host_t, dev_t):
                h.copy_(d, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            self._pending.append((host_t, ev, (boxes, scores, counts, gt_d, gc_d, fl_d, gb_d, ga_d, dcb_d, dcc_d, cal_d, hw_d, mh_d,
                                                status, matched, sim, rows, on, ws)))
            first = len(self._tags)
            self._tags += [f"{first + b:06d}" for b in range(B)] if tags is None else [str(t) for t in tags]
            self._n_valid += n_valid.sum(axis=0)

    def _batches(self):
        """the host copies of every batch, waited for: (status, matched, similarity, rows, on_image, scores) NumPy"""
        for i, (host_t, ev, _) in enumerate(self._pending):
            ev.synchronize()
            self._pending[i] = (host_t, ev, ())          # the device side of this batch is done
            yield tuple(t.numpy() for t in host_t)

    def compute(self):
        n_diff = len(self.difficulties)
        scores = [np.zeros(0, dtype=np.float32)]
        status = [[[np.zeros(0, dtype=np.int8)] for _ in range(n_diff)] for _ in KITTI_METRICS]
        sims = [[np.zeros(0, dtype=np.float64)] for _ in range(n_diff)]
        n_ignored = np.zeros(n_diff, dtype=np.int64)
        for st, mg, sm, _, _, sc in self._batches():
            there = st[:, 0, 0, :] != EMPTY          # the slots below the frame's count: same for every matching
            scores.append(sc[there])
            for k in range(n_diff):
                for m in range(len(KITTI_METRICS)):
                    status[m][k].append(st[:, m, k, :][there])
                sims[k].append(sm[:, k, :][there])
                n_ignored[k] += int(((st[:, 2, k, :] == IGNORED) & (mg[:, 2, k, :] < 0))[there].sum())
        sc = np.concatenate(scores)
        out = {"n_gt": {d: int(self._n_valid[k]) for k, d in enumerate(self.difficulties)}, "n_det": int(sc.size),
               "n_ignored": {d: int(n_ignored[k]) for k, d in enumerate(self.difficulties)}}
        for m, metric in enumerate(KITTI_METRICS):
            out[metric] = {d: average_precision(sc, np.concatenate(status[m][k]), self._n_valid[k], self.recall_points)
                           for k, d in enumerate(self.difficulties)}
        bbox = KITTI_METRICS.index("bbox")
        out["aos"] = {d: average_orientation_similarity(sc, np.concatenate(status[bbox][k]), np.concatenate(sims[k]),
                                                        self._n_valid[k], self.recall_points)
                      for k, d in enumerate(self.difficulties)}
        return out

    def result_lines(self, tags=None):
        """-> (tags, lines): per frame fed so far, the KITTI result lines of its on-image detections, best score first
        (ties: lower index).  tags: replaces the remembered names (one per frame)."""
        names = list(self._tags) if tags is None else [str(t) for t in tags]
        if len(names) != len(self._tags):
            raise ValueError(f"{len(names)} tags for {len(self._tags)} frames")
        lines = []
        for st, _, _, rows, on, sc in self._batches():
            for b in range(st.shape[0]):
                idx = [d for d in range(st.shape[-1]) if st[b, 0, 0, d] != EMPTY and on[b, d]]
                idx.sort(key=lambda d: (-float(sc[b, d]), d))
                lines.append([format_result_line(self.cls_name, rows[b, d], sc[b, d]) for d in idx])
        return names, lines

    def write_results(self, directory, tags=None):
        """one <tag>.txt per frame in `directory` (created if missing); a frame without detections gets an empty file,
        because KITTI's tool wants one per frame.  -> the paths written"""
        os.makedirs(directory, exist_ok=True)
        paths = []
        for tag, lines in zip(*self.result_lines(tags)):
            path = os.path.join(directory, f"{tag}.txt")
            with open(path, "w") as fh:
                fh.write("".join(line + "\n" for line in lines))
            paths.append(path)
        return paths


def calib_source(calib):
    """RPN3D.evaluate's `calib` -> a callable tag -> (P2, Tr, R0) or None (the mean calibration): "mean", a directory of
    <tag>.txt KITTI calibration files, or a callable"""
    if isinstance(calib, str) and calib == "mean":
        return lambda tag: None
    if isinstance(calib, (str, os.PathLike)):
        return lambda tag: load_kitti_calib(os.path.join(calib, f"{tag}.txt"))
    if callable(calib):
        return calib
    raise ValueError('calib: "mean", a directory of <tag>.txt calibration files, or a callable tag -> (P2, Tr, R0)')
