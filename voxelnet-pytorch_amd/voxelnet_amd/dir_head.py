"""Direction-classifier head of the RPN (csrc/dir_head.hip): a Conv2d(768, 2, 1) on the concatenation gives
one logit per anchor in the site layout of prob, dir[b, a, s]; its binary cross-entropy against the heading bin of the
matched box supervises the sign the sine yaw loss leaves open, and the decode turns a detection's yaw
into the half-plane the logit names.  Four library calls; there is no CPU path."""
import math

import torch

from . import _lib
from ._site_term import SiteTermFn, check_site_maps

C_CAT = 768
DIR_OFFSET = math.pi / 4


def check_spec(dir_weight=0.2, dir_offset=DIR_OFFSET):
    """ValueError for a weight / offset the head cannot run with — what the library would answer with VN_EINVAL, raised on
    the host before anything is launched."""
    for name, v in (("dir_weight", dir_weight), ("dir_offset", dir_offset)):
        try:
            ok = math.isfinite(float(v))
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError(f"{name} must be a finite number, not {v!r}")


def _need_hip(what, **ts):
    for name, t in ts.items():
        if not (torch.is_tensor(t) and t.is_cuda):
            raise _lib.VoxelnetHipError(f"{what}: {name} must be a tensor on a HIP device (no CPU path)")


def _flat(what, name, rows):
    """(B, S, width) rows whose samples follow each other at the row stride -> the (B*S, width) view; 2-D rows pass"""
    if torch.is_tensor(rows) and rows.dim() == 3:
        if rows.stride(2) != 1 or rows.stride(0) != rows.shape[1] * rows.stride(1):
            raise ValueError(f"{what}: {name} {tuple(rows.shape)} / strides {tuple(rows.stride())} is not one row matrix")
        return rows.as_strided((rows.shape[0] * rows.shape[1], rows.shape[2]), (rows.stride(1), 1))
    return rows


def _rows(what, name, rows):
    """(M, >= 768) bf16 / fp32 rows with a unit channel stride -> (vnDtype, row stride in elements)"""
    if rows.dim() != 2 or rows.shape[1] < C_CAT or rows.stride(1) != 1 or rows.stride(0) < C_CAT:
        raise ValueError(f"{what}: {name} {tuple(rows.shape)} / strides {tuple(rows.stride())} is not (M, >= {C_CAT}) rows")
    if rows.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"{what}: {name} must be float32 or bfloat16, not {rows.dtype}")
    return (_lib.VN_F32 if rows.dtype == torch.float32 else _lib.VN_BF16), rows.stride(0)


def _weights(what, weight, bias):
    if weight.numel() != 2 * C_CAT or weight.shape[0] != 2 or weight.dtype != torch.float32:
        raise ValueError(f"{what}: weight {tuple(weight.shape)} {weight.dtype} is not (2, {C_CAT}[, 1, 1]) float32")
    if bias is not None and (tuple(bias.shape) != (2,) or bias.dtype != torch.float32):
        raise ValueError(f"{what}: bias {tuple(bias.shape)} {bias.dtype} is not (2,) float32")


def dir_head_forward(cat_rows, weight, bias=None, B=None):
    """cat_rows (B, S, >= 768) — or (B*S, >= 768) with B given — bf16 / fp32 rows (the first 768 columns are read), weight
    (2, 768[, 1, 1]) and bias (2,) or None fp32 -> logits (B, 2, S) fp32: vn_dir_head_fwd."""
    if B is None and torch.is_tensor(cat_rows):
        B = cat_rows.shape[0] if cat_rows.dim() == 3 else 1
    cat_rows = _flat("dir_head_forward", "cat_rows", cat_rows)
    _need_hip("dir_head_forward", cat_rows=cat_rows, weight=weight, **({} if bias is None else {"bias": bias}))
    dt, stride = _rows("dir_head_forward", "cat_rows", cat_rows)
    _weights("dir_head_forward", weight, bias)
    M = cat_rows.shape[0]
    if not (isinstance(B, int) and B > 0 and M > 0 and M % B == 0):
        raise ValueError(f"dir_head_forward: {M} rows are not B = {B!r} samples")
    S = M // B
    w = weight.detach().contiguous()
    logits = torch.empty((B, 2, S), dtype=torch.float32, device=cat_rows.device)
    with _lib.on_device(cat_rows.device):
        _lib.call("vn_dir_head_fwd", cat_rows.data_ptr(), dt, stride, w.data_ptr(),
                  bias.detach().contiguous().data_ptr() if bias is not None else None, B, S, logits.data_ptr(), _lib.raw_stream())
    return logits


def dir_head_backward(d_logits, cat_rows, weight, d_cat):
    """d_logits (B, 2, S) fp32; cat_rows as in the forward; d_cat (B*S, >= 768) bf16 / fp32 rows, updated IN PLACE at the rows
    whose gradient is not zero (d_cat[m] += g0 w[0] + g1 w[1]; every other row is not touched) -> (d_weight (2, 768), d_bias (2,))
    fp32: vn_dir_head_bwd.  cat_rows and d_cat may be (B, S, width) as well."""
    cat_rows, d_cat = _flat("dir_head_backward", "cat_rows", cat_rows), _flat("dir_head_backward", "d_cat", d_cat)
    _need_hip("dir_head_backward", d_logits=d_logits, cat_rows=cat_rows, weight=weight, d_cat=d_cat)
    dt, stride = _rows("dir_head_backward", "cat_rows", cat_rows)
    ddt, dstride = _rows("dir_head_backward", "d_cat", d_cat)
    _weights("dir_head_backward", weight, None)
    if d_logits.dim() != 3 or d_logits.shape[1] != 2 or d_logits.dtype != torch.float32:
        raise ValueError(f"dir_head_backward: d_logits {tuple(d_logits.shape)} {d_logits.dtype} is not (B, 2, S) float32")
    B, _, S = d_logits.shape
    if cat_rows.shape[0] != B * S or d_cat.shape[0] != B * S or B * S == 0:
        raise ValueError(f"dir_head_backward: {cat_rows.shape[0]} / {d_cat.shape[0]} rows for a gradient of {B} x {S} sites")
    dev = d_logits.device
    g, w = d_logits.contiguous(), weight.detach().contiguous()
    d_w = torch.empty((2, C_CAT), dtype=torch.float32, device=dev)
    d_b = torch.empty(2, dtype=torch.float32, device=dev)
    with _lib.on_device(dev):
        nbytes = _lib.load().vn_dir_head_bwd_workspace_bytes(B, S)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        _lib.call("vn_dir_head_bwd", g.data_ptr(), cat_rows.data_ptr(), dt, stride, w.data_ptr(), B, S, d_cat.data_ptr(), ddt,
                  dstride, d_w.data_ptr(), d_b.data_ptr(), ws.data_ptr(), nbytes, _lib.raw_stream())
    return d_w, d_b


def rpn_dir_loss(dir_logits, pos, targets, anchors, dir_offset=DIR_OFFSET):
    """dir_logits (B,2,H*W) or (B,2,H,W) — the head's output —, pos (B,H,W,2), targets (B,H,W,14) fp32 and anchors (H*W*2, 7)
    or (H,W,2,7) float64, all HIP tensors -> (loss, acc) device scalars: include/voxelnet_hip.h, vn_rpn_dir_loss.  loss
    carries the gradient to dir_logits (_site_term.SiteTermFn; a gradient of 0 stays +0: what vn_dir_head_bwd skips); acc — the
    share of positives whose logit names the right bin — is a diagnostic."""
    check_spec(0.0, dir_offset)
    _need_hip("rpn_dir_loss", dir_logits=dir_logits, pos=pos, targets=targets, anchors=anchors)
    if pos.dim() != 4 or pos.shape[3] != 2:
        raise ValueError(f"rpn_dir_loss: pos {tuple(pos.shape)} is not (B,H,W,2)")
    B, H, W, _ = pos.shape
    x_ok = dir_logits.dim() in (3, 4) and dir_logits.shape[:2] == (B, 2) and dir_logits[0, 0].numel() == H * W
    check_site_maps("rpn_dir_loss", dir_logits, x_ok, pos, targets, anchors, B, H, W)
    if not dir_logits.is_floating_point():
        raise ValueError(f"rpn_dir_loss: dir_logits must be a floating-point tensor, not {dir_logits.dtype}")
    pos, targets, anchors = pos.contiguous(), targets.contiguous(), anchors.contiguous()

    def launch(z, out2, d_logits):
        ws_bytes = _lib.load().vn_rpn_dir_loss_workspace_bytes(B, H, W)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=z.device)
        _lib.call("vn_rpn_dir_loss", z.data_ptr(), pos.data_ptr(), targets.data_ptr(), anchors.data_ptr(), B, H, W, float(dir_offset),
                  ws.data_ptr(), ws_bytes, out2.data_ptr(), None if d_logits is None else d_logits.data_ptr(), _lib.raw_stream())
    return SiteTermFn.apply(dir_logits, launch)


def rectify_yaw(boxes, idx, counts, dir_logits, n_anchors, dir_offset=DIR_OFFSET):
    """boxes (B,K,7) fp32, updated IN PLACE and returned; idx (B,K) int32 the anchor index n = 2 * site + rotation of every row
    (BoxDecoder.candidates_device with layout="site"), counts (B,) int32, dir_logits (B,2,n_anchors/2): column 6 of the first
    min(counts[b], K) rows becomes wrap_pi(r - dir_offset) + dir_offset + pi * [logit > 0]: vn_boxes_rectify_yaw."""
    check_spec(0.0, dir_offset)
    _need_hip("rectify_yaw", boxes=boxes, idx=idx, counts=counts, dir_logits=dir_logits)
    if boxes.dim() != 3 or boxes.shape[2] != 7 or boxes.dtype != torch.float32 or not boxes.is_contiguous():
        raise ValueError(f"rectify_yaw: boxes {tuple(boxes.shape)} {boxes.dtype} is not a contiguous (B,K,7) float32 tensor")
    B, K, _ = boxes.shape
    if tuple(idx.shape) != (B, K) or tuple(counts.shape) != (B,) or idx.dtype != torch.int32 or counts.dtype != torch.int32:
        raise ValueError(f"rectify_yaw: idx {tuple(idx.shape)} {idx.dtype} / counts {tuple(counts.shape)} {counts.dtype}: want "
                         f"int32 ({B},{K}) and ({B},)")
    if not isinstance(n_anchors, int) or n_anchors <= 0 or n_anchors % 2:
        raise ValueError(f"rectify_yaw: n_anchors must be a positive even integer, not {n_anchors!r}")
    if dir_logits.dim() < 2 or dir_logits.shape[:2] != (B, 2) or dir_logits.numel() != B * n_anchors or dir_logits.dtype != torch.float32:
        raise ValueError(f"rectify_yaw: dir_logits {tuple(dir_logits.shape)} {dir_logits.dtype} is not ({B},2,{n_anchors // 2}) float32")
    if B == 0 or K == 0:
        return boxes
    with _lib.on_device(boxes.device):
        _lib.call("vn_boxes_rectify_yaw", boxes.data_ptr(), idx.contiguous().data_ptr(), counts.contiguous().data_ptr(),
                  dir_logits.detach().contiguous().data_ptr(), B, K, n_anchors, float(dir_offset), _lib.raw_stream())
    return boxes
