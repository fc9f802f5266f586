"""Rotated-IoU regression loss of the RPN (csrc/iou_loss.hip): 1 - IoU or the DIoU form between the box every
positive anchor's regression channels decode to and the box its target decodes to, bird's-eye view or 3D.  One library
call gives the two scalars and the gradient; there is no CPU path."""
import math

import torch

from . import _lib

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


class _IouLossFn(torch.autograd.Function):
    """vn_rpn_iou_loss -> (loss, mean_iou).  The forward launch writes d_delta for an upstream gradient of 1 and keeps it;
    backward multiplies it by the upstream scalar.  mean_iou is a diagnostic without a gradient."""

    @staticmethod
    def forward(ctx, delta, pos, tgt, anchors, kind, metric):
        B, C, H, W = delta.shape
        d32 = delta.detach().contiguous().float()
        need = ctx.needs_input_grad[0]
        with _lib.on_device(d32.device):
            ws_bytes = _lib.load().vn_rpn_iou_loss_workspace_bytes(B, H, W)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=d32.device)
            out = torch.empty(2, dtype=torch.float32, device=d32.device)
            d_delta = torch.empty_like(d32) if need else None
            _lib.call("vn_rpn_iou_loss", d32.data_ptr(), pos.data_ptr(), tgt.data_ptr(), anchors.data_ptr(), B, H, W, kind, metric,
                      None, ws.data_ptr(), ws_bytes, out.data_ptr(), d_delta.data_ptr() if need else None, _lib.raw_stream())
        ctx.d_delta, ctx.dtype = d_delta, delta.dtype
        ctx.set_materialize_grads(False)
        loss, mean_iou = out[0], out[1]          # (views of one buffer, as _LossFn's five)
        ctx.mark_non_differentiable(mean_iou)
        return loss, mean_iou

    @staticmethod
    def backward(ctx, g_loss, _g_iou):
        if g_loss is None or ctx.d_delta is None:
            return None, None, None, None, None, None
        return (ctx.d_delta * g_loss.float()).to(ctx.dtype), None, None, None, None, None


def rpn_iou_loss(delta, pos, targets, anchors, kind="iou", metric="3d"):
    """delta (B,14,H,W) — the module's regression output —, pos (B,H,W,2), targets (B,H,W,14) fp32 and anchors (H*W*2, 7)
    or (H,W,2,7) float64, all HIP tensors -> (loss, mean_iou) device scalars: include/voxelnet_hip.h, vn_rpn_iou_loss.
    loss carries the gradient to delta; mean_iou — the positives' mean IoU — is a diagnostic."""
    check_spec(kind, metric)
    for name, t in (("delta", delta), ("pos", pos), ("targets", targets), ("anchors", anchors)):
        if not (torch.is_tensor(t) and t.is_cuda):
            raise _lib.VoxelnetHipError(f"rpn_iou_loss: {name} must be a tensor on a HIP device (no CPU path)")
    if delta.dim() != 4 or delta.shape[1] != 14:
        raise ValueError(f"rpn_iou_loss: delta {tuple(delta.shape)} is not (B,14,H,W)")
    B, _, H, W = delta.shape
    if tuple(pos.shape) != (B, H, W, 2) or tuple(targets.shape) != (B, H, W, 14) or anchors.numel() != H * W * 14:
        raise ValueError(f"rpn_iou_loss: shapes {tuple(delta.shape)} {tuple(pos.shape)} {tuple(targets.shape)} "
                         f"{tuple(anchors.shape)} do not belong together")
    if anchors.dtype != torch.float64 or pos.dtype != torch.float32 or targets.dtype != torch.float32:
        raise ValueError("rpn_iou_loss: pos and targets must be float32, anchors float64")
    if not (pos.device == targets.device == anchors.device == delta.device):
        raise ValueError("rpn_iou_loss: the four tensors must live on one device")
    return _IouLossFn.apply(delta, pos.contiguous(), targets.contiguous(), anchors.contiguous(), KINDS[kind], METRICS[metric])
