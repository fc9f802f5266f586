"""Inference tail of the reference's `RPN3D.predict` (voxelnet/model.py:364-395) on the device: box decoding
(utils.deltas_to_boxes_3d, utils.py:476-489), score filter, stand-up rectangles and NMS (model.filter_boxes,
model.py:28-57; utils.nms, utils.py:492-553) through `vn_rpn_predict` (csrc/predict.hip).  The probability and delta
maps never leave HBM; only the <= NMS_POST_TOPK kept boxes per sample come back.  No CPU fallback.

For evaluation the same tail with the three steps an average precision needs (csrc/detect.hip): a
pre-NMS top-K in the thousands, a greedy NMS on stand-up rectangles or on the rotated footprints, a post-NMS cap —
`decode_device(..., nms=, pre_nms_top_k=)` through `vn_rpn_detect`, and its two halves on their own:
`BoxDecoder.candidates_device` (`vn_rpn_select_decode`) and `nms_device` (`vn_box_nms`).

`layout=`: "flat" reads the maps as the reference's reshape without a permute does; "site" reads
them as the loss trains them — anchor (site, rotation a) is scored by probs[b, a, site] and decoded from
deltas[b, 7a .. 7a+6, site] — through `vn_rpn_detect_layout` / `vn_rpn_select_decode_layout`.  A model trained by this
package's loss has to be decoded with layout="site": `TRAINED_DECODE`.

`dir_logits=`: the direction head's map (B,2,h,w) turns every detection's yaw into the half-plane its
anchor's logit names (`dir_head.rectify_yaw`); the tail is then composed from the public pieces — candidates, the yaw
rectification, `nms_device`, a gather of the kept rows — and needs layout="site".

`anchor_mask=`: a (B,h,w,2) uint8 mask of `anchor_mask.AnchorMasker` — an anchor without voxels under
its footprint scores 0 in a copy of the probability map (`vn_anchor_mask_probs`), and every tail above runs unchanged on it.

`iou_logits=`: the IoU-aware head's map (B,2,h,w) — every anchor is scored by p^(1 - iou_rectify) *
sigmoid(z)^iou_rectify in a copy of the probability map (`iou_head.rectify_probs`), made BEFORE the anchor mask edits that
copy; every tail above runs unchanged on it, score_thres applies to the rectified score, and it needs layout="site".

`vote=`: a `tta.BoxVote` — the composed tail ends in `tta.vote_device` (`vn_box_vote`) instead of the
gather: every kept row becomes the weighted mean of the candidates that overlap it.

`soft_nms=`: a `SoftNMS` — the composed tail runs `soft_nms_device` (`vn_box_soft_nms`) in place of
`nms_device`: a kept row decays the scores of the rows it overlaps instead of deleting them, and the kept rows come back with
their decayed scores."""
import ctypes
import math
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _lib
from .targets import CLASS_CFG, generate_anchors

SCORE_THRES, NMS_THRES, NMS_POST_TOPK = 0.96, 0.1, 20          # config.py:95-98 (cfg.RPN)
NMS_MODES = {"standup": _lib.VN_NMS_STANDUP, "rotated": _lib.VN_NMS_ROTATED}
# A starting point for RPN3D.evaluate(decode=...), NOT tuned: there is no trained checkpoint here to tune it on.
EVAL_DECODE = dict(score_thres=0.1, nms="rotated", nms_thres=0.1, pre_nms_top_k=1024)
LAYOUTS = {"flat": _lib.VN_DETECT_FLAT, "site": _lib.VN_DETECT_SITE}
SOFT_METHODS = {"hard": _lib.VN_SOFT_HARD, "linear": _lib.VN_SOFT_LINEAR, "gaussian": _lib.VN_SOFT_GAUSSIAN}
SOFT_METRICS = {"bev": _lib.VN_SOFT_BEV, "3d": _lib.VN_SOFT_3D}
# EVAL_DECODE in the layout the loss trains: RPN3D.evaluate(decode=TRAINED_DECODE) for a model trained here
TRAINED_DECODE = dict(EVAL_DECODE, layout="site")


def _nms_mode(nms):
    if nms not in NMS_MODES:
        raise ValueError(f"nms must be one of {sorted(NMS_MODES)}, not {nms!r}")
    return NMS_MODES[nms]


def _layout(layout):
    if layout not in LAYOUTS:
        raise ValueError(f"layout must be one of {sorted(LAYOUTS)}, not {layout!r}")
    return LAYOUTS[layout]


def _check_range(name, v, hi):
    if not (isinstance(v, (int, np.integer)) and 1 <= v <= hi):
        raise ValueError(f"{name} must be an integer in [1, {hi}], not {v!r}")
    return int(v)


def nms_device(boxes, counts, mode="rotated", nms_thres=NMS_THRES, top_k=NMS_POST_TOPK):
    """Greedy suppression as an operation of its own (vn_box_nms): boxes (B,K,7) f32 device tensor whose row order is the
    priority order, counts (B,) int32 device tensor (read on the device; above K means K) -> (keep_idx (B,top_k) int32, the
    kept row numbers in walk order, -1 past the count; keep_counts (B,) int32), on the device, no host synchronisation.
    mode "standup": vn_rpn_predict's rule; "rotated": the BEV IoU of evaluate.box_iou_rotated, rows with a non-finite
    field or h, w, l <= 0 are never kept."""
    if not (boxes.is_cuda and counts.is_cuda):
        raise _lib.VoxelnetHipError("nms_device: boxes / counts must be HIP tensors (no CPU path)")
    m = _nms_mode(mode)
    if boxes.dim() != 3 or boxes.shape[2] != 7 or counts.shape != (boxes.shape[0],) or boxes.shape[0] < 1:
        raise ValueError(f"boxes {tuple(boxes.shape)} / counts {tuple(counts.shape)}: want (B,K,7) and (B,)")
    B, K = boxes.shape[0], _check_range("K", boxes.shape[1], _lib.VN_DETECT_MAX_PRE)
    top_k = _check_range("top_k", top_k, _lib.VN_PREDICT_MAX_TOPK)
    if not np.isfinite(nms_thres):
        raise ValueError("nms_thres must be finite")
    boxes, counts = boxes.detach().float().contiguous(), counts.to(torch.int32).contiguous()
    dev = boxes.device
    keep = torch.empty((B, top_k), dtype=torch.int32, device=dev)
    kc = torch.empty(B, dtype=torch.int32, device=dev)
    nbytes = _lib.load().vn_box_nms_workspace_bytes(B, K)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    with _lib.on_device(dev):
        _lib.call("vn_box_nms", boxes.data_ptr(), counts.data_ptr(), B, K, m, float(nms_thres), top_k, keep.data_ptr(),
                  kc.data_ptr(), ws.data_ptr(), nbytes, _lib.raw_stream())
    return keep, kc


def _is_real(v):
    return isinstance(v, (int, float, np.floating, np.integer)) and not isinstance(v, (bool, np.bool_)) and math.isfinite(v)


@dataclass(frozen=True)
class SoftNMS:
    """Soft-NMS (vn_box_soft_nms).  method: "gaussian" (w *= exp(-IoU^2 / sigma) for every IoU > 0), "linear"
    (w *= 1 - IoU above iou_thres) or "hard" (a row above iou_thres is removed: the greedy rule); metric: the "bev" or the "3d"
    IoU of evaluate.box_iou_rotated; sigma > 0 is read by "gaussian", iou_thres in [0, 1] by "linear" and "hard"; min_score: the
    walk stops at the first pick whose decayed score is below it (None: the decode call's score_thres).  Not tuned: there is
    no trained checkpoint here to tune it on."""
    method: str = "gaussian"
    sigma: float = 0.5
    iou_thres: float = 0.3
    metric: str = "bev"
    min_score: Optional[float] = None

    def __post_init__(self):
        if self.method not in SOFT_METHODS:
            raise ValueError(f"SoftNMS.method must be one of {sorted(SOFT_METHODS)}, not {self.method!r}")
        if self.metric not in SOFT_METRICS:
            raise ValueError(f"SoftNMS.metric must be one of {sorted(SOFT_METRICS)}, not {self.metric!r}")
        if not (_is_real(self.sigma) and self.sigma > 0):
            raise ValueError(f"SoftNMS.sigma must be finite and > 0, not {self.sigma!r}")
        if not (_is_real(self.iou_thres) and 0 <= self.iou_thres <= 1):
            raise ValueError(f"SoftNMS.iou_thres must be in [0, 1], not {self.iou_thres!r}")
        if self.min_score is not None and not _is_real(self.min_score):
            raise ValueError(f"SoftNMS.min_score must be finite or None, not {self.min_score!r}")


def soft_nms_device(boxes, scores, counts, soft, top_k=NMS_POST_TOPK, min_score=None):
    """Soft-NMS as an operation of its own (vn_box_soft_nms): boxes (B,K,7) f32, scores (B,K) f32, counts (B,) int32 device
    tensors (counts read on the device; above K means K), soft: a SoftNMS -> (keep_idx (B,top_k) int32, the picked row numbers
    in pick order, -1 past the count; keep_scores (B,top_k) f32, their decayed scores, 0 past the count; keep_counts (B,) int32),
    on the device, no host synchronisation.  The rows need no order: every pick is an arg-max.  min_score: where the walk stops
    when soft.min_score is None (one of the two must be set).  Rows with a non-finite field, h, w, l <= 0 or a non-finite score
    are never kept and decay nothing."""
    if not isinstance(soft, SoftNMS):
        raise ValueError(f"soft must be a predict.SoftNMS, not {soft!r}")
    floor = soft.min_score if soft.min_score is not None else min_score
    if floor is None:
        raise ValueError("soft_nms_device: min_score is None and so is soft.min_score; one of them must say where the walk stops")
    if not _is_real(floor):
        raise ValueError(f"min_score must be finite, not {floor!r}")
    if not all(torch.is_tensor(t) and t.is_cuda for t in (boxes, scores, counts)):
        raise _lib.VoxelnetHipError("soft_nms_device: boxes / scores / counts must be HIP tensors (no CPU path)")
    if boxes.dim() != 3 or boxes.shape[2] != 7 or scores.shape != boxes.shape[:2] or counts.shape != (boxes.shape[0],) \
            or boxes.shape[0] < 1:
        raise ValueError(f"boxes {tuple(boxes.shape)} / scores {tuple(scores.shape)} / counts {tuple(counts.shape)}: want (B,K,7), "
                         "(B,K) and (B,)")
    B, K = boxes.shape[0], _check_range("K", boxes.shape[1], _lib.VN_DETECT_MAX_PRE)
    top_k = _check_range("top_k", top_k, _lib.VN_PREDICT_MAX_TOPK)
    boxes, scores = boxes.detach().float().contiguous(), scores.detach().float().contiguous()
    counts = counts.to(torch.int32).contiguous()
    dev = boxes.device
    keep = torch.empty((B, top_k), dtype=torch.int32, device=dev)
    ks = torch.empty((B, top_k), dtype=torch.float32, device=dev)
    kc = torch.empty(B, dtype=torch.int32, device=dev)
    nbytes = _lib.load().vn_box_soft_nms_workspace_bytes(B, K)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    with _lib.on_device(dev):
        _lib.call("vn_box_soft_nms", boxes.data_ptr(), scores.data_ptr(), counts.data_ptr(), B, K, SOFT_METHODS[soft.method],
                  SOFT_METRICS[soft.metric], float(soft.iou_thres), float(soft.sigma), float(floor), top_k, keep.data_ptr(),
                  ks.data_ptr(), kc.data_ptr(), ws.data_ptr(), nbytes, _lib.raw_stream())
    return keep, ks, kc


def gather_kept(boxes, scores, keep_idx, keep_counts, keep_scores=None):
    """the kept rows of a pool in vn_rpn_predict's output format -> (boxes (B,P,7), scores (B,P), keep_counts), rows past the
    count zero: the last step of every composed tail that ends in nms_device.  keep_scores (None: the pool's scores, gathered):
    soft_nms_device's (B,P) decayed scores, which then come back in place of the pool's — the one copy for every soft tail."""
    B, P = keep_idx.shape
    live = (keep_idx >= 0) & (torch.arange(P, device=keep_idx.device)[None, :] < keep_counts[:, None])
    rows = keep_idx.clamp(min=0).long()
    out = torch.gather(boxes, 1, rows[:, :, None].expand(B, P, 7))
    sc = torch.gather(scores, 1, rows) if keep_scores is None else keep_scores
    out = torch.where(live[:, :, None], out, torch.zeros_like(out))          # rows past the count are zero
    sc = torch.where(live, sc, torch.zeros_like(sc))
    return out, sc, keep_counts


class BoxDecoder:
    def __init__(self, cls_name="Car", device="cuda:0", anchors=None, layout="flat"):
        _layout(layout)
        self.cls_name = cls_name
        self.layout = layout          # the default of every call; each takes layout= of its own
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.VoxelnetHipError("BoxDecoder needs a HIP device (no CPU path)")
        self.anchors = generate_anchors(cls_name) if anchors is None else np.asarray(anchors, dtype=np.float64)
        self._anchors_dev = torch.from_numpy(np.ascontiguousarray(self.anchors.reshape(-1, 7))).to(self.device)
        self.n_anchors = self._anchors_dev.shape[0]
        self.anchor_h = float(CLASS_CFG[cls_name]["h"])

    def _maps(self, probs, deltas, what):
        if not (probs.is_cuda and deltas.is_cuda):
            raise _lib.VoxelnetHipError(f"{what}: probs / deltas must be HIP tensors (no CPU path)")
        probs, deltas = probs.detach().float().contiguous(), deltas.detach().float().contiguous()
        N = self.n_anchors
        if probs[0].numel() != N or deltas[0].numel() != 7 * N:
            raise ValueError(f"maps of {probs[0].numel()} / {deltas[0].numel()} elements do not match {N} anchors")
        return probs, deltas

    def _masked(self, probs, anchor_mask, score_thres, layout, what):
        """the copy of probs in which every anchor the mask (anchor_mask.AnchorMasker) leaves out scores 0, in the
        layout the decode reads: every tail below runs unchanged on it"""
        from .anchor_mask import mask_probs
        if not score_thres > 0:
            raise ValueError(f"{what}: anchor_mask needs score_thres > 0 (a masked-out anchor scores 0 and would be a candidate), "
                             f"not {score_thres!r}")
        lay = _layout(self.layout if layout is None else layout)
        if not (torch.is_tensor(probs) and probs.is_cuda):
            raise _lib.VoxelnetHipError(f"{what}: probs / deltas must be HIP tensors (no CPU path)")
        if torch.is_tensor(anchor_mask) and anchor_mask.is_cuda and (anchor_mask.dim() < 1 or anchor_mask.shape[0] != probs.shape[0]
                                                                     or anchor_mask.numel() != probs.shape[0] * self.n_anchors):
            raise ValueError(f"{what}: anchor_mask {tuple(anchor_mask.shape)} is not a mask of {probs.shape[0]} x {self.n_anchors} anchors")
        return mask_probs(probs.detach().float(), anchor_mask, self.n_anchors, lay)

    def _rectified(self, probs, iou_logits, iou_rectify, layout, what):
        """the copy of probs in which every anchor scores p^(1 - iou_rectify) * sigmoid(iou_logits)^iou_rectify:
        every tail below — and the anchor mask, which comes after it — runs unchanged on it"""
        from .iou_head import rectify_probs
        lay = self.layout if layout is None else layout
        if _layout(lay) != _lib.VN_DETECT_SITE:
            raise ValueError(f"iou_logits: the IoU-aware head's logits are laid out by site; layout must be 'site', not {lay!r}")
        if not (torch.is_tensor(probs) and probs.is_cuda):
            raise _lib.VoxelnetHipError(f"{what}: probs / deltas must be HIP tensors (no CPU path)")
        if not (torch.is_tensor(iou_logits) and iou_logits.is_cuda):
            raise _lib.VoxelnetHipError(f"{what}: iou_logits must be a HIP tensor (no CPU path)")
        B = probs.shape[0]
        if probs.numel() != B * self.n_anchors or iou_logits.shape[0] != B or iou_logits.numel() != B * self.n_anchors:
            raise ValueError(f"iou_logits {tuple(iou_logits.shape)} / probs {tuple(probs.shape)} do not match {B} samples of "
                             f"{self.n_anchors} anchors")
        return rectify_probs(probs, iou_logits, iou_rectify).view(probs.shape)

    def _decode_composed(self, probs, deltas, score_thres, nms_thres, top_k, nms, pre_nms_top_k, layout, dir_logits, dir_offset,
                         vote=None, soft_nms=None):
        """decode_device composed from the public pieces: vn_rpn_select_decode_layout -> (dir_logits) vn_boxes_rectify_yaw ->
        vn_box_nms -> (vote) vn_box_vote, or a gather of the kept rows.  With the direction head's logits the yaw changes by
        multiples of pi only, so the candidates, the kept set and the scores are those of the fused tail
        (vn_rpn_detect_layout) on the same maps; with a tta.BoxVote every kept row becomes the weighted mean of its cluster
        (DESIGN.md 1m).  With a SoftNMS vn_box_soft_nms stands in place of vn_box_nms and the gather takes its
        decayed scores; nms_thres is then not read."""
        _nms_mode(nms)
        if soft_nms is not None:
            if not isinstance(soft_nms, SoftNMS):
                raise ValueError(f"soft_nms must be a predict.SoftNMS, not {soft_nms!r}")
            if nms != "rotated":
                raise ValueError(f"soft_nms decays by the rotated IoU; nms must be 'rotated', not {nms!r}")
            if vote is not None:
                raise ValueError("soft_nms with vote: the vote's cluster around a soft-kept row is not defined; pass one of the two")
        lay = self.layout if layout is None else layout
        _layout(lay)
        if dir_logits is not None and _layout(lay) != _lib.VN_DETECT_SITE:
            raise ValueError(f"dir_logits: the direction head's logits are laid out by site; layout must be 'site', not {lay!r}")
        top_k = _check_range("top_k", top_k, _lib.VN_PREDICT_MAX_TOPK)
        pre = _check_range("pre_nms_top_k", top_k if pre_nms_top_k is None else pre_nms_top_k, _lib.VN_DETECT_MAX_PRE)
        if soft_nms is None and not np.isfinite(nms_thres):
            raise ValueError("nms_thres must be finite")
        if vote is not None:
            from .tta import BoxVote, vote_device
            if not isinstance(vote, BoxVote):
                raise ValueError(f"vote must be a tta.BoxVote, not {vote!r}")
        B = probs.shape[0]
        if dir_logits is not None:
            from .dir_head import rectify_yaw
            if not (torch.is_tensor(dir_logits) and dir_logits.is_cuda):
                raise _lib.VoxelnetHipError("predict: dir_logits must be a HIP tensor (no CPU path)")
            if dir_logits.shape[0] != B or dir_logits.numel() != B * self.n_anchors:
                raise ValueError(f"dir_logits {tuple(dir_logits.shape)} does not match {B} samples of {self.n_anchors} anchors")
            dl = dir_logits.detach().float().contiguous().view(B, 2, self.n_anchors // 2)
        cb, cs, idx, cc = self.candidates_device(probs, deltas, score_thres, pre, layout=lay)
        if dir_logits is not None:
            rectify_yaw(cb, idx, cc, dl, self.n_anchors, dir_offset)
        if soft_nms is not None:
            keep, ks, kc = soft_nms_device(cb, cs, cc, soft_nms, top_k, min_score=float(score_thres))
            return gather_kept(cb, cs, keep, kc, keep_scores=ks)
        keep, kc = nms_device(cb, cc, nms, nms_thres, top_k)
        if vote is not None:
            return vote_device(cb, cs, cc, keep, kc, vote)[:3]
        return gather_kept(cb, cs, keep, kc)

    def decode_device(self, probs, deltas, score_thres=SCORE_THRES, nms_thres=NMS_THRES, top_k=NMS_POST_TOPK, nms="standup",
                      pre_nms_top_k=None, layout=None, dir_logits=None, dir_offset=math.pi / 4, anchor_mask=None, iou_logits=None,
                      iou_rectify=0.5, vote=None, soft_nms=None):
        """probs (B,2,h,w), deltas (B,14,h,w) fp32 device tensors -> (boxes (B,top_k,7) f32, scores (B,top_k) f32, counts (B,)
        int32) ON THE DEVICE, enqueued on the current stream without any host synchronisation: per sample the first
        counts[b] rows are the kept detections in descending score, the rest is zero.  What evaluate.DetectionEvaluator
        consumes.
        nms="standup", pre_nms_top_k=None is the reference's tail (vn_rpn_predict: the top_k best candidates enter a
        stand-up-rectangle NMS).  Anything else goes through vn_rpn_detect: the pre_nms_top_k (default top_k) best
        candidates enter the NMS, on stand-up rectangles or, nms="rotated", on the rotated footprints; top_k caps what
        it keeps.  layout (None: the decoder's): "site" always goes through vn_rpn_detect_layout, with nms="standup",
        pre_nms_top_k=None too (the reference's tail read in the layout the loss trains).
        dir_logits (None: every path above exactly as it is): the direction head's (B,2,h,w) map, layout "site" only — column 6
        becomes wrap_pi(r - dir_offset) + dir_offset + pi * [logit > 0] through the composed tail; apart from that
        column the kept set and the scores are the ones of the call without it.
        anchor_mask (None: nothing new is allocated or launched): a (B,h,w,2) uint8 mask (anchor_mask.AnchorMasker) —
        every path above runs unchanged on a copy of probs in which a masked-out anchor scores 0; needs score_thres > 0.
        iou_logits (None: nothing new is allocated or launched): the IoU-aware head's (B,2,h,w) map, layout "site"
        only — every path above, the anchor mask included, runs on a copy of probs in which an anchor scores
        p^(1 - iou_rectify) * sigmoid(z)^iou_rectify, iou_rectify in [0, 1]; score_thres applies to that score.
        vote (None: every path above exactly as it is, nothing new is allocated or launched): a tta.BoxVote — the
        tail is composed, candidates_device -> nms_device -> tta.vote_device, and every kept row comes back as the weighted mean
        of the candidates that overlap it by vote.thres; every option above keeps its meaning, the rows come in descending
        output score.
        soft_nms (None: every path above exactly as it is, nothing new is allocated or launched): a SoftNMS — the
        tail is composed, candidates_device -> soft_nms_device -> gather_kept: a picked row decays the scores of the rows it
        overlaps instead of deleting them, and the rows come back in pick order with their DECAYED scores.  dir_logits,
        iou_logits, anchor_mask, layout and pre_nms_top_k keep their meaning; nms must be "rotated"; nms_thres is NOT read
        (soft_nms.iou_thres is); the walk stops below soft_nms.min_score, or below score_thres when that is None; together
        with vote it is a ValueError."""
        if iou_logits is not None:          # (before the mask: 0^0 = 1 would bring a masked-out anchor back at iou_rectify = 1)
            probs = self._rectified(probs, iou_logits, iou_rectify, layout, "predict")
        if anchor_mask is not None:
            probs = self._masked(probs, anchor_mask, score_thres, layout, "predict")
        if dir_logits is not None or vote is not None or soft_nms is not None:
            return self._decode_composed(probs, deltas, score_thres, nms_thres, top_k, nms, pre_nms_top_k, layout, dir_logits,
                                         dir_offset, vote, soft_nms)
        mode = _nms_mode(nms)
        lay = _layout(self.layout if layout is None else layout)
        probs, deltas = self._maps(probs, deltas, "predict")
        B, N = probs.shape[0], self.n_anchors
        dev = probs.device
        if pre_nms_top_k is not None or mode != _lib.VN_NMS_STANDUP or lay != _lib.VN_DETECT_FLAT:
            top_k = _check_range("top_k", top_k, _lib.VN_PREDICT_MAX_TOPK)
            pre = _check_range("pre_nms_top_k", top_k if pre_nms_top_k is None else pre_nms_top_k, _lib.VN_DETECT_MAX_PRE)
            if not np.isfinite(nms_thres):
                raise ValueError("nms_thres must be finite")
        boxes = torch.zeros((B, top_k, 7), dtype=torch.float32, device=dev)
        scores = torch.zeros((B, top_k), dtype=torch.float32, device=dev)
        counts = torch.zeros(B, dtype=torch.int32, device=dev)
        if pre_nms_top_k is None and mode == _lib.VN_NMS_STANDUP and lay == _lib.VN_DETECT_FLAT:
            nbytes = _lib.load().vn_rpn_predict_workspace_bytes(B, N)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            with _lib.on_device(dev):
                _lib.call("vn_rpn_predict", probs.data_ptr(), deltas.data_ptr(), self._anchors_dev.data_ptr(), B, N,
                          float(score_thres), float(nms_thres), int(top_k), self.anchor_h, boxes.data_ptr(), scores.data_ptr(),
                          counts.data_ptr(), ws.data_ptr(), nbytes, _lib.raw_stream())
            return boxes, scores, counts
        nbytes = _lib.load().vn_rpn_detect_workspace_bytes(B, N, pre)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        with _lib.on_device(dev):
            if lay == _lib.VN_DETECT_FLAT:
                _lib.call("vn_rpn_detect", probs.data_ptr(), deltas.data_ptr(), self._anchors_dev.data_ptr(), B, N,
                          float(score_thres), pre, mode, float(nms_thres), top_k, self.anchor_h, boxes.data_ptr(), scores.data_ptr(),
                          counts.data_ptr(), ws.data_ptr(), nbytes, _lib.raw_stream())
            else:
                _lib.call("vn_rpn_detect_layout", probs.data_ptr(), deltas.data_ptr(), self._anchors_dev.data_ptr(), B, N,
                          float(score_thres), pre, mode, float(nms_thres), top_k, self.anchor_h, boxes.data_ptr(), scores.data_ptr(),
                          counts.data_ptr(), ws.data_ptr(), nbytes, _lib.raw_stream(), lay)
        return boxes, scores, counts

    def candidates_device(self, probs, deltas, score_thres, pre_nms_top_k, layout=None, dir_logits=None, dir_offset=math.pi / 4,
                          anchor_mask=None, iou_logits=None, iou_rectify=0.5):
        """The first half of the tail on its own (vn_rpn_select_decode): per sample the min(M, pre_nms_top_k) best of the M
        candidates with p >= score_thres, decoded, in descending (score, flat index) order -> (boxes (B,pre,7) f32, scores
        (B,pre) f32, flat anchor indices (B,pre) int32, counts (B,) int32) on the device; rows past the count are zero.
        layout "site" (vn_rpn_select_decode_layout): the index is the anchor index n = 2 * site + rotation of the target maps.
        dir_logits (layout "site" only): the candidates' yaw is rectified by the direction head's map (dir_head.rectify_yaw).
        anchor_mask: as decode_device's — a masked-out anchor is never a candidate.
        iou_logits / iou_rectify: as decode_device's — the candidates are picked, ordered and scored by the rectified score."""
        if iou_logits is not None:
            probs = self._rectified(probs, iou_logits, iou_rectify, layout, "candidates")
        if anchor_mask is not None:
            probs = self._masked(probs, anchor_mask, score_thres, layout, "candidates")
        lay = _layout(self.layout if layout is None else layout)
        if dir_logits is not None and lay != _lib.VN_DETECT_SITE:
            raise ValueError("dir_logits: the direction head's logits are laid out by site; layout must be 'site'")
        probs, deltas = self._maps(probs, deltas, "candidates")
        pre = _check_range("pre_nms_top_k", pre_nms_top_k, _lib.VN_DETECT_MAX_PRE)
        B, N = probs.shape[0], self.n_anchors
        dev = probs.device
        boxes = torch.zeros((B, pre, 7), dtype=torch.float32, device=dev)
        scores = torch.zeros((B, pre), dtype=torch.float32, device=dev)
        idx = torch.zeros((B, pre), dtype=torch.int32, device=dev)
        counts = torch.zeros(B, dtype=torch.int32, device=dev)
        nbytes = _lib.load().vn_rpn_select_decode_workspace_bytes(B, N, pre)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        with _lib.on_device(dev):
            if lay == _lib.VN_DETECT_FLAT:
                _lib.call("vn_rpn_select_decode", probs.data_ptr(), deltas.data_ptr(), self._anchors_dev.data_ptr(), B, N,
                          float(score_thres), pre, self.anchor_h, boxes.data_ptr(), scores.data_ptr(), idx.data_ptr(),
                          counts.data_ptr(), ws.data_ptr(), nbytes, _lib.raw_stream())
            else:
                _lib.call("vn_rpn_select_decode_layout", probs.data_ptr(), deltas.data_ptr(), self._anchors_dev.data_ptr(), B, N,
                          float(score_thres), pre, self.anchor_h, boxes.data_ptr(), scores.data_ptr(), idx.data_ptr(),
                          counts.data_ptr(), ws.data_ptr(), nbytes, _lib.raw_stream(), lay)
        if dir_logits is not None:
            from .dir_head import rectify_yaw
            if not (torch.is_tensor(dir_logits) and dir_logits.is_cuda):
                raise _lib.VoxelnetHipError("candidates: dir_logits must be a HIP tensor (no CPU path)")
            if dir_logits.shape[0] != B or dir_logits.numel() != B * N:
                raise ValueError(f"dir_logits {tuple(dir_logits.shape)} does not match {B} samples of {N} anchors")
            rectify_yaw(boxes, idx, counts, dir_logits.detach().float().contiguous().view(B, 2, N // 2), N, dir_offset)
        return boxes, scores, idx, counts

    def __call__(self, probs, deltas, score_thres=SCORE_THRES, nms_thres=NMS_THRES, top_k=NMS_POST_TOPK, nms="standup",
                 pre_nms_top_k=None, layout=None, dir_logits=None, dir_offset=math.pi / 4, anchor_mask=None, iou_logits=None,
                 iou_rectify=0.5, vote=None, soft_nms=None):
        """probs (B,2,h,w), deltas (B,14,h,w) fp32 device tensors -> ([boxes (n_i,7) f32 numpy], [scores (n_i,) f32 numpy])"""
        boxes, scores, counts = self.decode_device(probs, deltas, score_thres, nms_thres, top_k, nms, pre_nms_top_k, layout,
                                                   dir_logits, dir_offset, anchor_mask, iou_logits, iou_rectify, vote, soft_nms)
        B = boxes.shape[0]
        cnt = counts.cpu().numpy()
        bh, sh = boxes.cpu().numpy(), scores.cpu().numpy()
        return [bh[b, :cnt[b]].copy() for b in range(B)], [sh[b, :cnt[b]].copy() for b in range(B)]
