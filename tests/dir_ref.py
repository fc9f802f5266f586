"""Float64 restatement of the direction-classifier head: NumPy for the heading bin and the decode,
torch.nn.functional.binary_cross_entropy_with_logits in float64 with autograd for the loss (no derivative is written
out here), a plain matrix product for the 1x1 convolution.  Shares no code with the library or voxelnet_amd/dir_head.py.

  wrap_pi(x) = x - floor(x / pi) * pi                      in [0, pi)
  bin(theta) = int(floor((theta - dir_offset) / pi)) & 1
  theta_gt   = targets[b, s, 7a + 6] + anchors[2s + a, 6]   (the float32 target widened)
  L_dir      = sum_b (1 / P_b) sum over positives bce(dir[b, a, s], bin(theta_gt)),  P_b = max(1, sum pos[b])
  decode     r' = wrap_pi(r - dir_offset) + dir_offset + pi * [logit > 0]"""
import numpy as np
import torch
import torch.nn.functional as F

DIR_OFFSET = np.pi / 4
EDGE, ZERO = 1e-6, 1e-6          # the guard: no angle this close to a bin edge, no deciding logit this close to 0


def wrap_pi(x):
    x = np.asarray(x, dtype=np.float64)
    return x - np.floor(x / np.pi) * np.pi


def dir_bin(theta, dir_offset=DIR_OFFSET):
    theta = np.asarray(theta, dtype=np.float64)
    return np.floor((theta - dir_offset) / np.pi).astype(np.int64) & 1


def edge_gap(theta, dir_offset=DIR_OFFSET):
    """distance of wrap_pi(theta - dir_offset) from the nearer bin edge (0 or pi)"""
    w = wrap_pi(np.asarray(theta, dtype=np.float64) - dir_offset)
    return np.minimum(w, np.pi - w)


def theta_gt(targets, anchors):
    """targets (B,h,w,14) float32, anchors (h,w,2,7) or (h*w*2,7) float64 -> (B,h,w,2) float64"""
    t = np.asarray(targets)
    B, h, w, _ = t.shape
    r = np.asarray(anchors, dtype=np.float64).reshape(h, w, 2, 7)[..., 6]
    return t[..., [6, 13]].astype(np.float64) + r[None]


def site_layout(x):
    """(B,h,w,2) channels-last -> (B,2,h*w): the layout of the logits"""
    x = np.asarray(x)
    return np.ascontiguousarray(x.transpose(0, 3, 1, 2)).reshape(x.shape[0], 2, -1)


def guard(logits, pos, targets, anchors, dir_offset=DIR_OFFSET, exact_zeros=0):
    """asserts, on the reference alone, that no positive's angle lies within EDGE of a bin edge and no positive's logit
    within ZERO of 0 apart from `exact_zeros` logits that are exactly 0 -> (smallest edge gap, smallest |logit| != 0)"""
    m = site_layout(pos) != 0
    gap = site_layout(edge_gap(theta_gt(targets, anchors), dir_offset))[m]
    z = np.asarray(logits, dtype=np.float64).reshape(m.shape)[m]
    assert gap.size == 0 or gap.min() > EDGE, gap.min()
    assert int((z == 0).sum()) == exact_zeros, int((z == 0).sum())
    nz = np.abs(z[z != 0])
    assert nz.size == 0 or nz.min() > ZERO, nz.min()
    return (float(gap.min()) if gap.size else np.inf), (float(nz.min()) if nz.size else np.inf)


def loss_torch(z, pos, targets, anchors, dir_offset=DIR_OFFSET):
    """z: a float64 torch tensor (B,2,S) that may carry an autograd graph; the rest NumPy -> (L_dir as a torch scalar,
    the positives' mask (B,2,S), the bins (B,2,S))"""
    m = torch.from_numpy(site_layout(np.asarray(pos, dtype=np.float64)))
    t = torch.from_numpy(site_layout(dir_bin(theta_gt(targets, anchors), dir_offset)).astype(np.float64))
    per = F.binary_cross_entropy_with_logits(z, t, reduction="none") * (m != 0)
    p_b = m.sum(dim=(1, 2)).clamp(min=1.0)
    return (per.sum(dim=(1, 2)) / p_b).sum(), m, t


def loss(logits, pos, targets, anchors, dir_offset=DIR_OFFSET, with_grad=True):
    """logits (B,2,S) (any float array), pos (B,h,w,2), targets (B,h,w,14), anchors -> (L_dir, acc, d L_dir / d logits
    (B,2,S) float64 or None, (hits, positives))"""
    z = torch.tensor(np.asarray(logits, dtype=np.float64).reshape(np.asarray(pos).shape[0], 2, -1), requires_grad=with_grad)
    L, m, t = loss_torch(z, pos, targets, anchors, dir_offset)
    grad = None
    if with_grad:
        L.backward()
        grad = z.grad.numpy()
    zz, mm, tt = z.detach().numpy(), m.numpy() != 0, t.numpy()
    hits = int((((zz > 0) == (tt == 1)) & mm).sum())
    n = int(mm.sum())
    return float(L.detach()), hits / max(1, n), grad, (hits, n)


def rectify(r, logit, dir_offset=DIR_OFFSET):
    r = np.asarray(r, dtype=np.float64)
    return wrap_pi(r - dir_offset) + dir_offset + np.pi * (np.asarray(logit) > 0)


def head_forward(x, w, bias=None):
    """x (M,768), w (2,768), bias (2,) -> (M,2) float64 and the bound's sum_c |x_c w_c| (M,2)"""
    x, w = np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64).reshape(2, -1)
    out = x @ w.T
    if bias is not None:
        out = out + np.asarray(bias, dtype=np.float64)[None]
    return out, np.abs(x) @ np.abs(w).T


def head_backward(g, x, w, d_cat):
    """g (M,2), x (M,768), w (2,768), d_cat (M,768), all widened to float64 -> (d_cat + g w, d_w (2,768), d_bias (2,),
    sum |terms| of d_w (2,768), of d_bias (2,))"""
    g, x = np.asarray(g, dtype=np.float64), np.asarray(x, dtype=np.float64)
    w, d = np.asarray(w, dtype=np.float64).reshape(2, -1), np.asarray(d_cat, dtype=np.float64)
    return d + g @ w, g.T @ x, g.sum(axis=0), np.abs(g).T @ np.abs(x), np.abs(g).sum(axis=0)
