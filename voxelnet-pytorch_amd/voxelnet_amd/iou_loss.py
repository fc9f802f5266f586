"""Rotated-IoU regression loss of the RPN (csrc/iou_loss.hip): 1 - IoU or the DIoU form between the box every
positive anchor's regression channels decode to and the box its target decodes to, bird's-eye view or 3D.  One library
call gives the two scalars and the gradient; there is no CPU path."""
import math

import torch

from . import _lib
from ._site_term import SiteTermFn, check_site_maps

KINDS = {"iou": _lib.VN_IOU_LOSS_IOU, "diou": _lib.VN_IOU_LOSS_DIOU}
METRICS = {"bev": _lib.VN_IOU_BEV, "3d": _lib.VN_IOU_3D}


def check_spec(kind, metric="3d", weight=1.0):
    """ValueError for a kind / metric / weight the term cannot run with — what the library would answer with VN_EINVAL,
    raised on the host before anything is launched.  kind None (the term is off) passes with any other value."""
    if kind is None:
        return
    if kind not in KINDS:
        raise ValueError(f"iou_loss must be None, 'iou' or 'diou', not {kind!r}")
    if metric not in METRICS:
        raise ValueError(f"iou_metric must be 'bev' or '3d', not {metric!r}")
    try:
        ok = math.isfinite(float(weight))
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"iou_weight must be a finite number, not {weight!r}")


def rpn_iou_loss(delta, pos, targets, anchors, kind="iou", metric="3d"):
    """delta (B,14,H,W) — the module's regression output —, pos (B,H,W,2), targets (B,H,W,14) fp32 and anchors (H*W*2, 7)
    or (H,W,2,7) float64, all HIP tensors -> (loss, mean_iou) device scalars: include/voxelnet_hip.h, vn_rpn_iou_loss.
    loss carries the gradient to delta (the launch writes it for an upstream gradient of 1, _site_term.SiteTermFn scales it);
    mean_iou — the positives' mean IoU — is a diagnostic without one."""
    check_spec(kind, metric)
    for name, t in (("delta", delta), ("pos", pos), ("targets", targets), ("anchors", anchors)):
        if not (torch.is_tensor(t) and t.is_cuda):
            raise _lib.VoxelnetHipError(f"rpn_iou_loss: {name} must be a tensor on a HIP device (no CPU path)")
    if delta.dim() != 4 or delta.shape[1] != 14:
        raise ValueError(f"rpn_iou_loss: delta {tuple(delta.shape)} is not (B,14,H,W)")
    B, _, H, W = delta.shape
    check_site_maps("rpn_iou_loss", delta, True, pos, targets, anchors, B, H, W)
    pos, targets, anchors = pos.contiguous(), targets.contiguous(), anchors.contiguous()

    def launch(d32, out2, d_delta):
        ws_bytes = _lib.load().vn_rpn_iou_loss_workspace_bytes(B, H, W)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=d32.device)
        _lib.call("vn_rpn_iou_loss", d32.data_ptr(), pos.data_ptr(), targets.data_ptr(), anchors.data_ptr(), B, H, W, KINDS[kind],
                  METRICS[metric], None, ws.data_ptr(), ws_bytes, out2.data_ptr(), None if d_delta is None else d_delta.data_ptr(),
                  _lib.raw_stream())
    return SiteTermFn.apply(delta, launch)
