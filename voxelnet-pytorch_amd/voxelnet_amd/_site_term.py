"""What the RPN loss terms summed over the anchor sites share on the Python side (csrc/rpn_common.h's scaffold below them):
iou_loss.rpn_iou_loss and dir_head.rpn_dir_loss are one autograd Function around their library call and one set of rules
for the maps they read."""
import torch

from . import _lib


class SiteTermFn(torch.autograd.Function):
    """x, launch -> (loss, diagnostic).  launch(x32, out2, d_x) makes the library call on the contiguous fp32 copy of x; d_x
    is a buffer like x32, or None when x needs no gradient.  The call writes d_x for an upstream gradient of 1 and the
    Function keeps it; backward multiplies it by the upstream scalar (0 stays +0).  The diagnostic has no gradient."""

    @staticmethod
    def forward(ctx, x, launch):
        x32 = x.detach().contiguous().float()
        with _lib.on_device(x32.device):
            out2 = torch.empty(2, dtype=torch.float32, device=x32.device)
            d_x = torch.empty_like(x32) if ctx.needs_input_grad[0] else None
            launch(x32, out2, d_x)
        ctx.d_x, ctx.dtype, ctx.shape = d_x, x.dtype, x.shape
        ctx.set_materialize_grads(False)
        loss, diag = out2[0], out2[1]          # (views of one buffer, as _LossFn's five)
        ctx.mark_non_differentiable(diag)
        return loss, diag

    @staticmethod
    def backward(ctx, g_loss, _g_diag):
        if g_loss is None or ctx.d_x is None:
            return None, None
        return (ctx.d_x * g_loss.float()).to(ctx.dtype).view(ctx.shape), None


def check_site_maps(what, x, x_ok, pos, targets, anchors, B, H, W):
    """ValueError unless pos is (B,H,W,2) and targets (B,H,W,14) float32, anchors float64 with H*W*14 elements, and the
    three live on the device of x — the term's own tensor, whose shape the caller has judged (x_ok).  `what` names the
    caller in the messages."""
    if not x_ok or tuple(pos.shape) != (B, H, W, 2) or tuple(targets.shape) != (B, H, W, 14) or anchors.numel() != H * W * 14:
        raise ValueError(f"{what}: shapes {tuple(x.shape)} {tuple(pos.shape)} {tuple(targets.shape)} "
                         f"{tuple(anchors.shape)} do not belong together")
    if anchors.dtype != torch.float64 or pos.dtype != torch.float32 or targets.dtype != torch.float32:
        raise ValueError(f"{what}: pos and targets must be float32, anchors float64")
    if not (pos.device == targets.device == anchors.device == x.device):
        raise ValueError(f"{what}: the four tensors must live on one device")
