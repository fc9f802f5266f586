"""Reference for the RPN loss with a focal classification term and / or a sine yaw term (include/voxelnet_hip.h,
vnLossSpec), restated from the formulas in torch ops on whatever dtype it is handed (the tests hand it
float64): torch.pow, torch.sin and autograd — no derivative is written out here, and nothing is shared with the kernel's
algebra.  The regression term is the oracle's smooth_l1 (the reference's quirk included) on the masked difference.

  P_b     = max(1, sum pos[b])                                   N_b = max(1, sum neg[b])
  focal:    cls_pos = fa * pos * (1-p)^gamma * (-log(p + eps)) / P_b
            cls_neg = (1-fa) * neg * p^gamma * (-log(1 - p + eps)) / P_b          (over P_b, not N_b)
  bce:      cls_pos = pos * (-log(p + eps)) / P_b ;  cls_neg = neg * (-log(1 - p + eps)) / N_b      (the reference's)
  diff_j  = pos * (delta_j - tgt_j), j = 0..5;   diff_6 = pos * (delta_6 - tgt_6)  or  pos * sin(delta_6 - tgt_6)
  reg     = smooth_L1(diff) / P_b
  -> (alpha*S_pos + beta*S_neg + S_reg, alpha*S_pos + beta*S_neg, S_reg, S_pos, S_neg)
"""
import torch

from oracle import torch_ref as tr

EPS = 1e-6


def loss(prob, delta, pos, neg, targets, alpha=1.5, beta=1.0, sigma=3.0, cls="focal", fa=0.25, gamma=2.0, yaw="diff"):
    """prob (B,2,h,w), delta (B,14,h,w); pos, neg (B,h,w,2), targets (B,h,w,14) channels-last -> the five scalars"""
    assert cls in ("focal", "bce") and yaw in ("diff", "sin")
    B, _, h, w = prob.shape
    p_b = pos.sum(dim=(1, 2, 3)).clamp(min=1).reshape(B, 1, 1, 1)
    n_b = neg.sum(dim=(1, 2, 3)).clamp(min=1).reshape(B, 1, 1, 1)
    pos_c, neg_c = pos.permute(0, 3, 1, 2), neg.permute(0, 3, 1, 2)                 # (B,2,h,w)
    nll_pos, nll_neg = -torch.log(prob + EPS), -torch.log(1 - prob + EPS)
    if cls == "focal":
        cls_pos = fa * pos_c * torch.pow(1 - prob, gamma) * nll_pos / p_b
        cls_neg = (1 - fa) * neg_c * torch.pow(prob, gamma) * nll_neg / p_b
    else:
        cls_pos = pos_c * nll_pos / p_b
        cls_neg = neg_c * nll_neg / n_b
    s_pos, s_neg = cls_pos.sum(), cls_neg.sum()
    d = delta.reshape(B, 2, 7, h, w) - targets.permute(0, 3, 1, 2).reshape(B, 2, 7, h, w)      # anchor-major channels
    if yaw == "sin":
        d = torch.cat([d[:, :, :6], torch.sin(d[:, :, 6:])], dim=2)
    d = d * pos_c.unsqueeze(2)
    s_reg = (tr.smooth_l1(d, torch.zeros_like(d), sigma) / p_b.unsqueeze(1)).sum()
    c = alpha * s_pos + beta * s_neg
    return c + s_reg, c, s_reg, s_pos, s_neg
