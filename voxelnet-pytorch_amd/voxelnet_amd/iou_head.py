"""IoU-aware confidence head of the RPN (csrc/iou_head.hip): a second Conv2d(768, 2, 1) on the concatenation
gives one logit per anchor in the site layout of prob, z[b, a, s]; q = sigmoid(z) is trained (a binary cross-entropy with a
soft target) to predict the IoU of the anchor's decoded box with its ground truth, and the decode ranks a detection by
p^(1 - alpha) q^alpha instead of p.  The head's forward and backward are dir_head's; there is no CPU path."""
import math

import torch

from . import _lib
from ._site_term import SiteTermFn, check_site_maps
from .dir_head import C_CAT, _flat, _need_hip, _rows, _weights
from .iou_loss import METRICS


def check_spec(iou_head_weight=1.0, iou_rectify=0.5, iou_head_metric="3d"):
    """ValueError for a weight / exponent / metric the head cannot run with — what the library would answer with VN_EINVAL,
    raised on the host before anything is launched."""
    try:
        ok = math.isfinite(float(iou_head_weight))
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"iou_head_weight must be a finite number, not {iou_head_weight!r}")
    try:
        ok = 0.0 <= float(iou_rectify) <= 1.0          # (False for a NaN)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"iou_rectify must be a number in [0, 1], not {iou_rectify!r}")
    if iou_head_metric not in METRICS:
        raise ValueError(f"iou_head_metric must be 'bev' or '3d', not {iou_head_metric!r}")


def rpn_iou_head_loss(logits, delta, pos, targets, anchors, metric="3d", return_target=False):
    """logits (B,2,H*W) or (B,2,H,W) — the head's output —, delta (B,14,H,W) — the regression output, read DETACHED: the target
    is a constant —, pos (B,H,W,2), targets (B,H,W,14) fp32 and anchors (H*W*2, 7) or (H,W,2,7) float64, all HIP tensors ->
    (loss, mae) device scalars: include/voxelnet_hip.h, vn_rpn_iou_head_loss.  loss carries the gradient to logits
    (_site_term.SiteTermFn; a gradient of 0 stays +0: what vn_dir_head_bwd skips); mae — the positives' mean |sigmoid(z) - IoU| —
    is a diagnostic.  return_target: a third result, the target map (B,2,H*W) fp32, +0 where pos is 0."""
    check_spec(0.0, 0.0, metric)
    _need_hip("rpn_iou_head_loss", logits=logits, delta=delta, pos=pos, targets=targets, anchors=anchors)
    if pos.dim() != 4 or pos.shape[3] != 2:
        raise ValueError(f"rpn_iou_head_loss: pos {tuple(pos.shape)} is not (B,H,W,2)")
    B, H, W, _ = pos.shape
    x_ok = (logits.dim() in (3, 4) and logits.shape[:2] == (B, 2) and logits[0, 0].numel() == H * W
            and tuple(delta.shape) == (B, 14, H, W) and delta.device == logits.device)
    check_site_maps("rpn_iou_head_loss", logits, x_ok, pos, targets, anchors, B, H, W)
    if not (logits.is_floating_point() and delta.is_floating_point()):
        raise ValueError(f"rpn_iou_head_loss: logits and delta must be floating-point tensors, not {logits.dtype} / {delta.dtype}")
    pos, targets, anchors = pos.contiguous(), targets.contiguous(), anchors.contiguous()
    d32 = delta.detach().contiguous().float()
    t_map = torch.empty((B, 2, H * W), dtype=torch.float32, device=logits.device) if return_target else None

    def launch(z, out2, d_logits):
        ws_bytes = _lib.load().vn_rpn_iou_head_loss_workspace_bytes(B, H, W)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=z.device)
        _lib.call("vn_rpn_iou_head_loss", z.data_ptr(), d32.data_ptr(), pos.data_ptr(), targets.data_ptr(), anchors.data_ptr(), B, H, W,
                  METRICS[metric], ws.data_ptr(), ws_bytes, out2.data_ptr(), None if d_logits is None else d_logits.data_ptr(),
                  None if t_map is None else t_map.data_ptr(), _lib.raw_stream())
    loss, mae = SiteTermFn.apply(logits, launch)
    return (loss, mae, t_map) if return_target else (loss, mae)


def rectify_probs(probs, iou_logits, alpha):
    """probs and iou_logits of B * 2 * S elements each, both in the site layout (probs[b, a, s]) -> a NEW fp32 tensor shaped
    like probs: p^(1 - alpha) * sigmoid(z)^alpha, both powers float64 (vn_iou_rectify_probs); alpha = 0 gives p's bits."""
    check_spec(0.0, alpha)
    _need_hip("rectify_probs", probs=probs, iou_logits=iou_logits)
    if iou_logits.numel() != probs.numel() or iou_logits.device != probs.device:
        raise ValueError(f"rectify_probs: iou_logits {tuple(iou_logits.shape)} does not match probs {tuple(probs.shape)}")
    p = probs.detach().float().contiguous()
    z = iou_logits.detach().float().contiguous()
    out = torch.empty_like(p)
    if p.numel() == 0:
        return out
    with _lib.on_device(p.device):
        _lib.call("vn_iou_rectify_probs", p.data_ptr(), z.data_ptr(), p.numel(), float(alpha), out.data_ptr(), _lib.raw_stream())
    return out


def site_heads_forward(cat_rows, weights, biases, B=None):
    """The forward of one or two Conv2d(768, 2, 1) heads in ONE read of the rows (vn_site_heads_fwd): cat_rows as
    dir_head.dir_head_forward's, weights a sequence of one or two (2, 768[, 1, 1]) fp32 tensors, biases a sequence of as many
    (2,) tensors or None (all or none) -> a tuple of (B, 2, S) fp32 logits, one per head, each bit for bit what
    dir_head_forward gives for that head alone."""
    what = "site_heads_forward"
    weights = list(weights)
    biases = [None] * len(weights) if biases is None else list(biases)
    if len(weights) not in (1, 2) or len(biases) != len(weights):
        raise ValueError(f"{what}: {len(weights)} weights / {len(biases)} biases: want one or two heads")
    if any(b is None for b in biases) and not all(b is None for b in biases):
        raise ValueError(f"{what}: the heads have a bias all or none")
    if B is None and torch.is_tensor(cat_rows):
        B = cat_rows.shape[0] if cat_rows.dim() == 3 else 1
    cat_rows = _flat(what, "cat_rows", cat_rows)
    _need_hip(what, cat_rows=cat_rows, **{f"weight{i}": w for i, w in enumerate(weights)},
              **{f"bias{i}": b for i, b in enumerate(biases) if b is not None})
    dt, stride = _rows(what, "cat_rows", cat_rows)
    for w, b in zip(weights, biases):
        _weights(what, w, b)
    M = cat_rows.shape[0]
    if not (isinstance(B, int) and B > 0 and M > 0 and M % B == 0):
        raise ValueError(f"{what}: {M} rows are not B = {B!r} samples")
    S, n_out = M // B, 2 * len(weights)
    w = torch.cat([x.detach().reshape(2, C_CAT) for x in weights]).contiguous()
    bias = None if biases[0] is None else torch.cat([b.detach() for b in biases]).contiguous()
    logits = torch.empty((B, n_out, S), dtype=torch.float32, device=cat_rows.device)
    with _lib.on_device(cat_rows.device):
        _lib.call("vn_site_heads_fwd", cat_rows.data_ptr(), dt, stride, w.data_ptr(), None if bias is None else bias.data_ptr(),
                  n_out, B, S, logits.data_ptr(), _lib.raw_stream())
    return tuple(logits[:, 2 * i:2 * i + 2] for i in range(len(weights)))
