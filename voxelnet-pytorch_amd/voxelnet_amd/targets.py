"""RPN training targets — the reference's `generate_anchors` (voxelnet/utils.py:104-130) and `generate_targets`
(utils.py:376-473; called by RPN3D.forward, model.py:309) with the per-anchor work on the device (csrc/targets.hip,
`vn_rpn_targets`).

Host side (O(number of boxes) NumPy, as in the reference): KITTI label lines -> lidar boxes (utils.py:147-210), their
stand-up rectangles (utils.py:230-252, 283-330).  Device side: 70,400 anchors x boxes IoU with the reference's
conventions and quirks, the positive / negative assignment and the regression encoding.  Outputs stay on the device
in the layouts `RPN3D.loss` takes — no float64 host arrays, no six host-to-device copies per step (model.py:327-332).
There is no CPU fallback: the HIP library must be present.

`TargetGenerator(assign=)`: "reference" is that assignment, quirks included; "standup" and "rotated" assign by a real IoU
(csrc/targets_iou.hip, `vn_rpn_targets_iou`) — what a model that is to be evaluated has to be
trained with.  "atss" (csrc/targets_atss.hip, `vn_rpn_targets_atss`) drops the two fixed
thresholds: every box takes the `atss_top_k` nearest anchors of each rotation and sets its own threshold from their IoUs.
"simota" (csrc/targets_ota.hip, `vn_rpn_targets_ota`) is prediction-aware: it reads the network's
`probs` / `deltas` maps, and a box takes the anchors whose decoded prediction fits it best, as many as overlap it already."""
import ctypes
import os

import numpy as np
import torch

from . import _lib

MAX_GT = 128     # VN_TARGETS_MAX_GT (include/voxelnet_hip.h)
# assign -> vn_rpn_targets_iou's iou_kind (None: not that call — "reference" is vn_rpn_targets, "atss" vn_rpn_targets_atss,
# "simota" vn_rpn_targets_ota)
ASSIGN_KINDS = {"reference": None, "standup": _lib.VN_ASSIGN_STANDUP, "rotated": _lib.VN_ASSIGN_ROTATED, "atss": None,
                "simota": None}
ATSS_IOU_KINDS = {"standup": _lib.VN_ASSIGN_STANDUP, "rotated": _lib.VN_ASSIGN_ROTATED}
ATSS_MAX_TOPK = 32     # VN_ATSS_MAX_TOPK
OTA_METRICS = {"bev": _lib.VN_IOU_BEV, "3d": _lib.VN_IOU_3D}
OTA_MAX_Q = 16         # VN_OTA_MAX_Q
OTA_RADIUS_PITCHES = 2.5          # ota_radius=None: this many site pitches (YOLOX's centre radius, there in strides)

# voxelnet/config.py:36-92 (anchor geometry, IoU thresholds) and :99-111 (mean KITTI calibration)
CLASS_CFG = {
    "Car": dict(x=(0.0, 70.4), y=(-40.0, 40.0), fw=176, fh=200, l=3.9, w=1.6, h=1.56, z=-1.0 - 1.56 / 2, pos_iou=0.6,
                neg_iou=0.45, accept=("Car", "Van")),
    "Pedestrian": dict(x=(0.0, 48.0), y=(-20.0, 20.0), fw=120, fh=100, l=0.8, w=0.6, h=1.73, z=-0.6 - 1.73 / 2,
                       pos_iou=0.5, neg_iou=0.35, accept=("Pedestrian",)),
    "Cyclist": dict(x=(0.0, 48.0), y=(-20.0, 20.0), fw=120, fh=100, l=1.76, w=0.6, h=1.73, z=-0.6 - 1.73 / 2,
                    pos_iou=0.5, neg_iou=0.35, accept=("Cyclist",)),
}
_T_VELO_2_CAM = np.array([[7.49916597e-03, -9.99971248e-01, -8.65110297e-04, -6.71807577e-03],
                          [1.18652889e-02, 9.54520517e-04, -9.99910318e-01, -7.33152811e-02],
                          [9.99882833e-01, 7.49141178e-03, 1.18719929e-02, -2.78557062e-01],
                          [0, 0, 0, 1]])
_R_RECT_0 = np.array([[0.99992475, 0.00975976, -0.00734152, 0],
                      [-0.0097913, 0.99994262, -0.00430371, 0],
                      [0.00729911, 0.0043753, 0.99996319, 0],
                      [0, 0, 0, 1]])
_R_RECT_0_INV, _T_VELO_2_CAM_INV = np.linalg.inv(_R_RECT_0), np.linalg.inv(_T_VELO_2_CAM)   # (utils.py:168-169 inverts per call)


def generate_anchors(cls_name="Car"):
    """utils.py:104-130: (FEATURE_HEIGHT, FEATURE_WIDTH, 2, 7) float64 anchors [x, y, z, h, w, l, r], r in {0, pi/2}."""
    c = CLASS_CFG[cls_name]
    gx, gy = np.meshgrid(np.linspace(c["x"][0], c["x"][1], c["fw"]), np.linspace(c["y"][0], c["y"][1], c["fh"]))
    a = np.empty((c["fh"], c["fw"], 2, 7))
    a[..., 0] = gx[..., None]
    a[..., 1] = gy[..., None]
    a[..., 2], a[..., 3], a[..., 4], a[..., 5] = c["z"], c["h"], c["w"], c["l"]
    a[..., 0, 6] = 0
    a[..., 1, 6] = 90 / 180 * np.pi
    return a


def _limit_angle(angle):
    """utils.py:133-144"""
    while angle >= np.pi / 2:
        angle -= np.pi
    while angle < -np.pi / 2:
        angle += np.pi
    return np.pi / 2 if abs(angle + np.pi / 2) < 5 / 180 * np.pi else angle


def _wrap_angle(angle):
    """into (-pi, pi]: the heading kept (what _limit_angle folds away), as evaluate.py reads a label's rotation_y"""
    return angle - 2.0 * np.pi * np.ceil((angle - np.pi) / (2.0 * np.pi))


def label_to_gt_box_3d(labels, cls_name="Car", coordinate="lidar", keep_heading=False):
    """utils.py:178-210 (+ camera_to_lidar_box, :163-174): label lines of every sample -> list of (G_i, 7) float64
    boxes (x, y, z, h, w, l, r), in lidar coordinates by the mean calibration unless coordinate == 'camera'.
    keep_heading: r = -ry - pi/2 wrapped into (-pi, pi] instead of the reference's fold into [-pi/2, pi/2), which
    forgets which way the object faces — what a direction head is supervised by."""
    accept = CLASS_CFG[cls_name]["accept"] if cls_name in CLASS_CFG else ()
    r_inv, t_inv = _R_RECT_0_INV, _T_VELO_2_CAM_INV
    out = []
    for label in labels:
        rows = []
        for line in label:
            f = line.split()
            if accept and f[0] not in accept:
                continue
            h, w, l, x, y, z, ry = (float(v) for v in f[-7:])
            if coordinate == "lidar":
                p = np.matmul(t_inv, np.matmul(r_inv, np.array([x, y, z, 1])))
                rows.append([p[0], p[1], p[2], h, w, l, (_wrap_angle if keep_heading else _limit_angle)(-ry - np.pi / 2)])
            else:
                rows.append([x, y, z, h, w, l, ry])
        out.append(np.array(rows, dtype=np.float64).reshape(-1, 7))
    return out


def lidar_box_to_label_line(cls_name, box):
    """inverse of label_to_gt_box_3d for one box (x, y, z, h, w, l, r) in lidar coordinates: the KITTI label line (camera
    coordinates by the mean calibration, utils.py lidar_to_camera) the dataset would hand to RPN3D.forward — synthetic
    labels for bench.py / tests"""
    x, y, z, h, w, l, rz = (float(v) for v in box)
    p = np.matmul(_R_RECT_0, np.matmul(_T_VELO_2_CAM, np.array([x, y, z, 1.0])))
    return (f"{cls_name} 0.00 0 0.00 0.00 0.00 0.00 0.00 {h:.2f} {w:.2f} {l:.2f} {p[0]:.2f} {p[1]:.2f} {p[2]:.2f} "
            f"{-rz - np.pi / 2:.2f}")


def gt_standup_boxes(gt):
    """corner_to_standup_box2d(center_to_corner_box_2d(gt[:, [0,1,4,5,6]])) (utils.py:402-406): axis-aligned hull of
    the rotated footprint; float64 rotation, corners stored as float32 (utils.py:293), result float32 (utils.py:410)."""
    out = np.zeros((gt.shape[0], 4), dtype=np.float32)
    for i, (x, y, _, _, w, l, yaw) in enumerate(gt):
        foot = np.array([[-l / 2, -l / 2, l / 2, l / 2], [w / 2, -w / 2, -w / 2, w / 2], [0.0, 0.0, 0.0, 0.0]])
        rot = np.array([[np.cos(yaw), -np.sin(yaw), 0.0], [np.sin(yaw), np.cos(yaw), 0.0], [0.0, 0.0, 1.0]])
        c = (np.dot(rot, foot) + np.array([[x], [y], [0.0]])).T.astype(np.float32)
        out[i] = (c[:, 0].min(), c[:, 1].min(), c[:, 0].max(), c[:, 1].max())
    return out


# host-side memo of label text -> boxes (VN_LABEL_CACHE=0: parse every time, as the reference does; the DEVICE target
# generation runs every step either way — only host work is remembered, and the step is GPU-bound: same point-clouds/s)
_LABEL_CACHE = os.environ.get("VN_LABEL_CACHE", "1") != "0"


def check_assign_params(assign, atss_top_k, atss_iou, ota_q, ota_radius, ota_iou_weight, ota_metric, name="assign"):
    """ValueError for an assignment kind, or an ATSS / SimOTA parameter outside vn_rpn_targets_atss's / vn_rpn_targets_ota's
    ranges (ota_radius None: derived from the anchors) — what TargetGenerator and RPN3D (name="target_assign") both check at
    construction, whatever the kind"""
    if assign not in ASSIGN_KINDS:
        raise ValueError(f"{name} must be one of {sorted(ASSIGN_KINDS)}, not {assign!r}")
    def int_in_range(what, v, hi):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= v <= hi:
            raise ValueError(f"{what} must be an int in 1..{hi}, not {v!r}")
    int_in_range("atss_top_k", atss_top_k, ATSS_MAX_TOPK)
    if atss_iou not in ATSS_IOU_KINDS:
        raise ValueError(f"atss_iou must be one of {sorted(ATSS_IOU_KINDS)}, not {atss_iou!r}")
    int_in_range("ota_q", ota_q, OTA_MAX_Q)
    for what, v in (("ota_radius", ota_radius), ("ota_iou_weight", ota_iou_weight)):
        if v is None and what == "ota_radius":
            continue
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not (0 <= v < float("inf")):
            raise ValueError(f"{what} must be a finite number >= 0, not {v!r}")
    if ota_metric not in OTA_METRICS:
        raise ValueError(f"ota_metric must be one of {sorted(OTA_METRICS)}, not {ota_metric!r}")


def site_pitch(anchors):
    """the anchor grid's site pitch in metres, read from an (h, w, 2, 7) anchor array: the larger of the mean column pitch
    (x) and the mean row pitch (y); ValueError for a grid of one site, which has none"""
    a = np.asarray(anchors, dtype=np.float64)
    h, w = a.shape[:2]
    pitches = ([abs(a[0, -1, 0, 0] - a[0, 0, 0, 0]) / (w - 1)] if w > 1 else []) + \
              ([abs(a[-1, 0, 0, 1] - a[0, 0, 0, 1]) / (h - 1)] if h > 1 else [])
    if not pitches or not np.isfinite(max(pitches)):
        raise ValueError("ota_radius=None needs an anchor grid of more than one site to read the pitch from: pass ota_radius")
    return float(max(pitches))


def check_maps(assign, probs, deltas, B, shape):
    """the rule of from_boxes' probs= / deltas=: both there, float32 and (B, 2, h, w) / (B, 14, h, w) under "simota"; neither
    under any other kind.  ValueError otherwise."""
    if assign != "simota":
        if probs is not None or deltas is not None:
            raise ValueError(f'probs= / deltas= belong to assign="simota": assign={assign!r} does not look at predictions')
        return
    if probs is None or deltas is None:
        raise ValueError('assign="simota" needs the prediction maps: probs=(B,2,h,w) and deltas=(B,14,h,w)')
    want = ((B, 2, *shape), (B, 14, *shape))
    for name, t, w in (("probs", probs, want[0]), ("deltas", deltas, want[1])):
        if not torch.is_tensor(t) or t.dtype != torch.float32:
            raise ValueError(f"{name} must be a float32 tensor, not {type(t).__name__ if not torch.is_tensor(t) else t.dtype}")
        if tuple(t.shape) != w:
            raise ValueError(f"{name} {tuple(t.shape)} is not the generator's grid: {w} expected")


class TargetGenerator:
    """Device-resident anchors of one class + the launch: `gen(labels)` -> (pos_equal_one (B,h,w,2), neg_equal_one
    (B,h,w,2), targets (B,h,w,14)) float32 tensors on `device`, the arrays of utils.generate_targets (utils.py:473).
    assign: "reference" — the reference's assignment (vn_rpn_targets); "standup" / "rotated" — by the IoU of the stand-up
    hulls / of the rotated footprints (vn_rpn_targets_iou), pos and neg then exclusive.  pos_iou /
    neg_iou: the two thresholds (default: the class's).  keep_heading: label lines are parsed with their heading
    (label_to_gt_box_3d), so that targets[..., 7a+6] + the anchor's yaw is the box's yaw and not its fold into [-pi/2, pi/2).
    assign "atss" (vn_rpn_targets_atss): per box the atss_top_k (1..32) nearest anchors of each rotation
    are its candidates, its threshold is the mean + standard deviation of their IoUs (atss_iou: "rotated" or "standup"), and a
    candidate at or above it whose centre lies inside the box is positive; every other anchor is negative.  pos_iou / neg_iou
    are accepted and IGNORED for "atss"; atss_top_k / atss_iou are checked always and used by "atss" only.
    assign "simota" (vn_rpn_targets_ota): needs from_boxes(..., probs=, deltas=), the module's fp32 NCHW
    outputs.  Per box the candidates are the anchors inside its footprint or within ota_radius metres of its centre along x
    and y (None: 2.5 site pitches of the anchor grid); it takes dyn_k = max(1, floor(sum of its ota_q largest IoUs between
    decoded prediction and box)) of them by the smallest cost -log p + ota_iou_weight * -log IoU (+1e5 outside footprint and
    radius both); an anchor two boxes select goes to the smaller cost.  ota_metric: "bev" or "3d".  pos_iou / neg_iou are
    ignored; the ota_* are checked always and used by "simota" only."""

    def __init__(self, cls_name="Car", device="cuda:0", anchors=None, assign="reference", pos_iou=None, neg_iou=None,
                 keep_heading=False, atss_top_k=9, atss_iou="rotated", ota_q=10, ota_radius=None, ota_iou_weight=3.0,
                 ota_metric="bev"):
        check_assign_params(assign, atss_top_k, atss_iou, ota_q, ota_radius, ota_iou_weight, ota_metric)
        # everything that defines this generator besides the device and the anchor grid, as given: RPN3D._target_generator
        # builds the same tuple from its own attributes and makes a new generator when the two differ
        self.key = (cls_name, assign, pos_iou, neg_iou, bool(keep_heading), atss_top_k, atss_iou, ota_q, ota_radius, ota_iou_weight,
                    ota_metric)
        self.atss_top_k, self.atss_iou = int(atss_top_k), atss_iou
        self.ota_q, self.ota_iou_weight, self.ota_metric = int(ota_q), float(ota_iou_weight), ota_metric
        self.ota_radius = None if ota_radius is None else float(ota_radius)
        self.cls_name = cls_name
        self.cfg = CLASS_CFG[cls_name]
        self.assign = assign
        self.keep_heading = bool(keep_heading)
        self.pos_iou = float(self.cfg["pos_iou"] if pos_iou is None else pos_iou)
        self.neg_iou = float(self.cfg["neg_iou"] if neg_iou is None else neg_iou)
        if np.isnan(self.pos_iou) or np.isnan(self.neg_iou):
            raise ValueError("pos_iou / neg_iou must not be NaN")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.VoxelnetHipError("TargetGenerator needs a HIP device (no CPU path)")
        self.anchors = generate_anchors(cls_name) if anchors is None else np.asarray(anchors, dtype=np.float64)
        self.shape = self.anchors.shape[:2]
        if assign == "simota" and self.ota_radius is None:
            self.ota_radius = OTA_RADIUS_PITCHES * site_pitch(self.anchors)
        self._anchors_dev = torch.from_numpy(np.ascontiguousarray(self.anchors.reshape(-1, 7))).to(self.device)
        self.n_anchors = self._anchors_dev.shape[0]
        self._parsed = {}          # (label lines, coordinate) -> (G, 7) float64 boxes
        self._standup = {}         # id-free cache of gt_standup_boxes, keyed by the boxes' bytes

    def _apply_mask(self, out, anchor_mask):
        """pos / neg of a fresh result with the anchors a (B,h,w,2) uint8 mask leaves out IGNORED — both zero:
        copies in which a kept entry is bit-identical (vn_anchor_mask_probs, flat: the maps are in anchor order); targets and
        matched stay as they are"""
        if anchor_mask is None:
            return out
        from .anchor_mask import mask_probs
        pos, neg = out[0], out[1]
        if torch.is_tensor(anchor_mask) and anchor_mask.is_cuda and tuple(anchor_mask.shape) != tuple(pos.shape):
            raise ValueError(f"anchor_mask {tuple(anchor_mask.shape)} is not the targets' {tuple(pos.shape)}")
        N = self.n_anchors
        return (mask_probs(pos, anchor_mask, N, _lib.VN_DETECT_FLAT), mask_probs(neg, anchor_mask, N, _lib.VN_DETECT_FLAT)) + tuple(out[2:])

    def _pack_boxes(self, gt_boxes, entry_name):
        """the samples' (G_i, 7) boxes as one zero-padded host array -> gt (B, G, 7) float64, cnt (B,) int32, B, G"""
        B = len(gt_boxes)
        G = max([b.shape[0] for b in gt_boxes] + [1])
        if G > MAX_GT:
            raise _lib.VoxelnetHipError(f"{G} ground-truth boxes in one sample; {entry_name} takes at most {MAX_GT}")
        gt = np.zeros((B, G, 7), dtype=np.float64)
        cnt = np.zeros(B, dtype=np.int32)
        for b, boxes in enumerate(gt_boxes):
            cnt[b] = boxes.shape[0]
            gt[b, :boxes.shape[0]] = boxes
        return gt, cnt, B, G

    def _standup_rects(self, gt_boxes, G):
        """the reference assignment's host-made (B, G, 4) float32 stand-up rectangles, remembered by the boxes' bytes"""
        g2 = np.zeros((len(gt_boxes), G, 4), dtype=np.float32)
        for b, boxes in enumerate(gt_boxes):
            n = boxes.shape[0]
            if n:
                key = boxes.tobytes()
                su = self._standup.get(key) if _LABEL_CACHE else None
                if su is None:
                    if len(self._standup) >= 8192:
                        self._standup.clear()
                    su = self._standup[key] = gt_standup_boxes(boxes)
                g2[b, :n] = su
        return g2

    def _outputs(self, B, return_matched):
        """fresh pos, neg (B,h,w,2), targets (B,h,w,14) float32 and, if wanted, matched (B,h,w,2) int32 (else None)"""
        new = lambda c, dtype: torch.empty((B, *self.shape, c), dtype=dtype, device=self.device)          # noqa: E731
        return new(2, torch.float32), new(2, torch.float32), new(14, torch.float32), new(2, torch.int32) if return_matched else None

    def _launch(self, name, ws_size_args, call_args):
        """entry point `name` on the generator's device and the current stream, with a workspace of the size its
        `name`_workspace_bytes(*ws_size_args) asks for appended to call_args"""
        nbytes = getattr(_lib.load(), name + "_workspace_bytes")(*ws_size_args)
        if nbytes == 0:
            raise _lib.VoxelnetHipError(f"{name}_workspace_bytes: unsupported sizes")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        with _lib.on_device(self.device):
            _lib.call(name, *call_args, ws.data_ptr(), nbytes, _lib.raw_stream())

    def from_boxes(self, gt_boxes, return_matched=False, anchor_mask=None, return_stats=False, probs=None, deltas=None):
        """gt_boxes: list of (G_i, 7) float64 lidar boxes per sample.  return_matched (every assign but "reference"): a fourth
        tensor (B,h,w,2) int32, every anchor's ground-truth index or -1.  return_stats (assign "atss" / "simota" only):
        appends the (B, G, 4) float64 tensor of every box's (mean, standard deviation, threshold, number of anchors matched to
        it) — under "simota" the (B, G, 5) tensor of (candidates, sum of the top IoUs, dyn_k, cost of the last selected
        candidate, anchors matched to it) —, zeros for a slot without a valid box.  probs / deltas (assign "simota" only, and
        required there): the module's (B,2,h,w) / (B,14,h,w) float32 outputs on the device, read on the current stream;
        ValueError when they are missing, given under another kind, or not the generator's grid.  anchor_mask (None: nothing new is launched): a
        (B,h,w,2) uint8 device mask (anchor_mask.AnchorMasker) — after the assignment, forced positives included,
        an anchor it leaves out is ignored: pos = neg = 0; targets and matched are not touched."""
        if return_stats and self.assign not in ("atss", "simota"):
            raise ValueError('return_stats needs assign="atss" or "simota": the other assignments have no per-box statistics')
        check_maps(self.assign, probs, deltas, len(gt_boxes), self.shape)
        ref, atss, ota = (self.assign == a for a in ("reference", "atss", "simota"))
        if ref and return_matched:
            raise ValueError('return_matched needs assign="standup", "rotated", "atss" or "simota": the reference assignment reports no index')
        name = "vn_rpn_targets" + ("" if ref else "_atss" if atss else "_ota" if ota else "_iou")
        gt, cnt, B, G = self._pack_boxes(gt_boxes, name)
        # "reference" alone needs the boxes' stand-up rectangles from the host; for every other kind everything per box
        # happens on the device too
        host = (gt, self._standup_rects(gt_boxes, G), cnt) if ref else (gt, cnt)
        dev, N = self.device, self.n_anchors
        # pinned staging + asynchronous copies on the current stream: a blocking copy from pageable memory would make the
        # host wait for everything queued before it — every step — and the train loop's enqueue could no longer run ahead
        # of the GPU (the caching host allocator keeps a pinned block until the copy that reads it has run)
        boxes_d = [torch.from_numpy(a).pin_memory().to(dev, non_blocking=True) for a in host]
        pos, neg, tgt, matched = self._outputs(B, return_matched)
        stats = torch.empty((B, G, 5 if ota else 4), dtype=torch.float64, device=dev) if return_stats else None
        if ref:
            mid, tail = (self.pos_iou, self.neg_iou), ()
        elif atss:
            mid, tail = (ATSS_IOU_KINDS[self.atss_iou], self.atss_top_k), (matched, stats)
        elif ota:
            if probs.device != dev or deltas.device != dev:
                raise ValueError(f"probs / deltas must live on the generator's device {dev}")
            probs, deltas = probs.contiguous(), deltas.contiguous()
            mid = (probs.data_ptr(), deltas.data_ptr(), OTA_METRICS[self.ota_metric], self.ota_q, self.ota_radius, self.ota_iou_weight)
            tail = (matched, stats)
        else:
            mid, tail = (ASSIGN_KINDS[self.assign], self.pos_iou, self.neg_iou), (matched,)
        self._launch(name, (B, N, G) + ((self.atss_top_k,) if atss else (self.ota_q,) if ota else ()),
                     (self._anchors_dev.data_ptr(), N, *(t.data_ptr() for t in boxes_d), B, G, *mid, float(self.cfg["h"]),
                      pos.data_ptr(), neg.data_ptr(), tgt.data_ptr(), *(None if t is None else t.data_ptr() for t in tail)))
        return self._apply_mask((pos, neg, tgt) + tuple(t for t in (matched, stats) if t is not None), anchor_mask)

    def __call__(self, labels, feature_map_shape=None, coordinate="lidar", anchor_mask=None, probs=None, deltas=None):
        if feature_map_shape is not None and tuple(feature_map_shape) != tuple(self.shape):
            raise ValueError(f"feature map {tuple(feature_map_shape)} does not match the anchors {tuple(self.shape)}")
        # label lines -> lidar boxes is a pure function of the TEXT of a sample's label: remembered per sample (an epoch
        # visits every sample's label once per epoch; 0.25 ms of the host's 1.8 ms per step went into re-parsing, NumPy
        # 4-vectors one box at a time — tools/host_cprofile.py).  Keyed by the text itself, not by object identity.
        boxes = []
        for label in labels:
            key = (tuple(label), coordinate)
            hit = self._parsed.get(key) if _LABEL_CACHE else None
            if hit is None:
                if len(self._parsed) >= 8192:
                    self._parsed.clear()
                hit = label_to_gt_box_3d([label], self.cls_name, coordinate, self.keep_heading)[0]
                hit.setflags(write=False)
                self._parsed[key] = hit
            boxes.append(hit)
        return self.from_boxes(boxes, anchor_mask=anchor_mask, probs=probs, deltas=deltas)


def generate_targets(labels, feature_map_shape, anchors, cls_name="Car", coordinate="lidar", device="cuda:0"):
    """utils.py:376-382 signature; returns device tensors instead of float64 host arrays."""
    return TargetGenerator(cls_name, device, anchors)(labels, feature_map_shape, coordinate)
