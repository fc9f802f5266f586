"""Float64 restatement of the IoU-aware confidence head: the target map from tests/iou_loss_ref.py's
decode and IoU (Sutherland-Hodgman on torch scalars), the soft-target binary cross-entropy with torch autograd, and the
rectified score in NumPy float64.  Nothing is shared with the library (voxelnet_amd is not imported).

Layouts: logits and every map returned here are in the site layout (B, 2, H*W): element [b, a, s] belongs to pos[b, y, x, a],
s = y * W + x."""
import numpy as np
import torch

import iou_loss_ref as IR

F64 = torch.float64


def site_layout(pos):
    """(B,H,W,2) -> (B,2,H*W)"""
    pos = np.asarray(pos)
    B, H, W, _ = pos.shape
    return np.ascontiguousarray(pos.reshape(B, H * W, 2).transpose(0, 2, 1))


def target_map(delta, pos, targets, anchors, metric="3d"):
    """-> (t (B,2,H*W) float64 numpy: clamp(IoU(decode(delta), decode(targets)), 0, 1) at the anchors with pos != 0 — 0 for an
    invalid pair — and 0 elsewhere; pairs, iou_loss_ref.loss' list).  Constants: nothing here is differentiated."""
    delta, pos, targets = (torch.as_tensor(np.asarray(v)) for v in (delta, pos, targets))
    B, _, H, W = delta.shape
    _, _, pairs = IR.loss(delta.detach(), pos, targets, torch.as_tensor(np.asarray(anchors)), "iou", metric)
    t = np.zeros((B, 2, H * W))
    for (b, y, x, a), iou, _ in pairs:
        t[b, a, y * W + x] = min(max(iou, 0.0), 1.0)
    return t, pairs


def bce_formula(z, t):
    """the definition's three terms, for VALUES only: autograd through max(z, 0) and |z| picks one-sided derivatives whose sum
    at z == 0 exactly is 1 - t, not sigmoid(0) - t"""
    return torch.clamp(z, min=0.0) - z * t + torch.log1p(torch.exp(-torch.abs(z)))


def bce(z, t):
    """the same function as torch's own operator, whose derivative is sigmoid(z) - t everywhere"""
    return torch.nn.functional.binary_cross_entropy_with_logits(z, t, reduction="none")


def loss_torch(logits, t, pos):
    """logits (B,2,S) torch float64 (may require grad), t (B,2,S) and pos (B,H,W,2) arrays -> (L, mae) torch scalars:
    L = sum_b (1 / max(1, sum pos[b])) sum m bce(z, t), mae = sum m |sigmoid(z) - t| / max(1, sum m)"""
    m = torch.from_numpy(site_layout(pos)).to(F64)
    t = torch.as_tensor(t, dtype=F64)
    B = m.shape[0]
    p_b = m.reshape(B, -1).sum(dim=1).clamp(min=1.0)
    L = ((m * bce(logits, t)).reshape(B, -1).sum(dim=1) / p_b).sum()
    mae = (m * (torch.sigmoid(logits.detach()) - t).abs()).sum() / m.sum().clamp(min=1.0)
    return L, mae


def loss(logits, delta, pos, targets, anchors, metric="3d"):
    """arrays -> (L, mae, d L / d logits (B,2,S) float64 numpy, t, pairs)"""
    t, pairs = target_map(delta, pos, targets, anchors, metric)
    z = torch.from_numpy(np.asarray(logits, dtype=np.float64)).clone().requires_grad_(True)
    L, mae = loss_torch(z, t, pos)
    L.backward()
    return float(L.detach()), float(mae), z.grad.numpy(), t, pairs


def rectify(p, z, alpha):
    """float32 p and z -> float32 (float64 pow(p, 1 - alpha) * pow(sigmoid(z), alpha)), rounded once"""
    p64, z64 = np.asarray(p, dtype=np.float64), np.asarray(z, dtype=np.float64)
    with np.errstate(over="ignore"):
        q = 1.0 / (1.0 + np.exp(-z64))
    return (np.power(p64, 1.0 - alpha) * np.power(q, alpha)).astype(np.float32)
