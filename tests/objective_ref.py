"""The full training objective of RPN3D, all terms at once, as ONE float64 function with autograd: a composition of the four
references the single-term tests already hold the kernels to — nothing is restated here.

  base      tests/focal_ref.loss            focal (or bce) classification + smooth-L1 regression with a sine (or diff) yaw
  L_iou     tests/iou_loss_ref.loss         the rotated-IoU / DIoU regression term
  L_dir     tests/dir_ref.loss_torch        the direction head's cross-entropy
  L_head    tests/iou_head_ref.target_map + loss_torch   the IoU-aware head's soft-target cross-entropy; its
            target is the IoU of the box the regression map decodes to, a CONSTANT (no gradient into the regression map)

  loss      = base.loss + iou_weight * L_iou + dir_weight * L_dir + iou_head_weight * L_head
  cls_loss  = base.cls  + dir_weight * L_dir + iou_head_weight * L_head
  reg_loss  = base.reg  + iou_weight * L_iou                                   (RPN3D.loss' five scalars; cls_pos / cls_neg as base)

`drop=` names ONE of the five terms to leave out — the reference a backward would equal that lost that term's contribution:
"dir", "iou_head", "iou" remove the term, "focal" falls back to bce and "sin" to the plain yaw difference.
tests/test_objective_host.py shows on this reference alone that each of the five moves every trunk gradient by at least
three times OBJECTIVE_BAR, the bar tests/test_gpu_objective.py holds all 108 device gradients to.

Does not import voxelnet_amd."""
import numpy as np
import torch
import torch.nn.functional as F

import dir_ref
import focal_ref
import iou_head_ref
import iou_loss_ref
from oracle import targets as ot
from oracle import torch_ref as tr

# Relative L2 every device gradient of the composed objective is held to against the frozen-mask float64 oracle
# (tests/test_gpu_objective.py::test_composed_objective_against_the_frozen_mask_oracle; measured worst there: 4.3e-5, under a
# third of the bar, which therefore stays at test_fp32_backward_chain_with_frozen_masks' 5e-4).
OBJECTIVE_BAR = 5e-4

TERMS = ("dir", "iou_head", "iou", "focal", "sin")
ANCHORS_TINY = np.ascontiguousarray(ot.generate_anchors("Car")[:8, :12])          # the 8 x 12 maps' anchors, (8,12,2,7) float64
TINY_DIMS = (10, 16, 24)
ABS = (1.5, 1.0, 3.0)                                                              # alpha, beta, sigma: the module's defaults
# the objective both test files build: the RPN3D keyword arguments of the switches (dir_weight: see test_objective_host)
MODEL_KW = dict(cls_loss="focal", focal_alpha=0.25, focal_gamma=2.0, yaw_loss="sin", iou_loss="diou", iou_weight=2.0,
                iou_metric="3d", dir_head=True, dir_weight=0.2, iou_head=True, iou_head_weight=1.0, iou_head_metric="3d")
HEAD_KEYS = ("middle_rpn.dir_conv.conv.weight", "middle_rpn.dir_conv.conv.bias",
             "middle_rpn.iou_conv.conv.weight", "middle_rpn.iou_conv.conv.bias")


def bn_fronted_bias(key):
    """a conv / deconv bias in front of a train-mode BatchNorm: its true gradient is exactly 0 (test_detect_fwd_bwd_fp32)"""
    return key.endswith("conv.bias") and not any(h in key for h in ("prob_conv", "reg_conv", "dir_conv", "iou_conv")) \
        or key.endswith("deconv.bias")


def guards(reg, dir_logits, iou_logits, pos, targets, anchors, dir_offset=dir_ref.DIR_OFFSET, metrics=("3d",)):
    """The conditions the single-term tests put on their reference inputs, asserted on float64 values alone:
    dir_ref.guard (no positive's heading within EDGE of a bin edge, no deciding logit within ZERO of 0), every positive's
    (decoded, target) pair of boxes valid for the IoU (iou_loss_ref._valid: finite, positive sizes), and at least one
    IoU-head target above 0.  -> dict of the figures"""
    reg, z_dir = reg.detach(), dir_logits.detach().numpy()
    B, _, H, W = reg.shape
    gap, zmin = dir_ref.guard(z_dir, pos, targets, anchors, dir_offset)
    A = torch.as_tensor(np.asarray(anchors), dtype=torch.float64).reshape(H, W, 2, 7)
    t64 = torch.as_tensor(np.asarray(targets), dtype=torch.float64)
    n_pairs = 0
    for b, y, x, a in np.argwhere(np.asarray(pos) != 0).tolist():
        P = iou_loss_ref.decode(reg[b, a * 7:a * 7 + 7, y, x], A[y, x, a])
        G = iou_loss_ref.decode(t64[b, y, x, a * 7:a * 7 + 7], A[y, x, a])
        for metric in metrics:
            assert iou_loss_ref._valid(P, G, metric), ((b, y, x, a), metric)
        n_pairs += 1
    assert n_pairs > 0
    t, _ = iou_head_ref.target_map(reg.numpy(), pos, targets, anchors, metrics[-1])
    assert t.max() > 0
    assert torch.isfinite(iou_logits.detach()).all()
    return dict(edge_gap=gap, min_logit=zmin, n_pairs=n_pairs, targets_above_0=int((t > 0).sum()), max_target=float(t.max()))


def objective(prob, reg, dir_logits, iou_logits, pos, neg, targets, anchors, *, alpha=ABS[0], beta=ABS[1], sigma=ABS[2],
              cls_loss="focal", focal_alpha=0.25, focal_gamma=2.0, yaw_loss="sin", iou_loss="diou", iou_metric="3d", iou_weight=2.0,
              dir_weight=0.2, dir_offset=dir_ref.DIR_OFFSET, iou_head_weight=1.0, iou_head_metric="3d", drop=None, guard=True):
    """prob (B,2,h,w), reg (B,14,h,w), dir_logits / iou_logits (B,2,h,w) or (B,2,h*w): float64 torch tensors that may carry
    an autograd graph; pos, neg (B,h,w,2), targets (B,h,w,14), anchors (h,w,2,7): arrays.
    -> dict: total (= loss), loss, cls_loss, reg_loss, cls_pos, cls_neg (the module's five scalars), terms = {focal, sin, iou,
    dir, iou_head} (unweighted: the classification sum, the regression sum, L_iou, L_dir, L_head; None where dropped),
    mean_iou, mae, guards."""
    assert drop is None or drop in TERMS, drop
    assert prob.dtype == reg.dtype == dir_logits.dtype == iou_logits.dtype == torch.float64
    B = prob.shape[0]
    pos_n, neg_n, tgt_n = (np.ascontiguousarray(np.asarray(v), dtype=np.float32) for v in (pos, neg, targets))
    pos_t, neg_t, tgt_t = (torch.from_numpy(v).double() for v in (pos_n, neg_n, tgt_n))
    z_dir, z_iou = dir_logits.reshape(B, 2, -1), iou_logits.reshape(B, 2, -1)
    out = dict(guards=guards(reg, z_dir, z_iou, pos_n, tgt_n, anchors, dir_offset,
                             tuple(dict.fromkeys((iou_metric, iou_head_metric)))) if guard else None)
    base = focal_ref.loss(prob, reg, pos_t, neg_t, tgt_t, alpha, beta, sigma, cls="bce" if drop == "focal" else cls_loss,
                          fa=focal_alpha, gamma=focal_gamma, yaw="diff" if drop == "sin" else yaw_loss)
    loss, cls, rg, cls_pos, cls_neg = base
    terms = dict(focal=None if drop == "focal" else cls, sin=None if drop == "sin" else rg, iou=None, dir=None, iou_head=None)
    out["mean_iou"] = out["mae"] = None
    if drop != "iou":
        l_iou, out["mean_iou"], _ = iou_loss_ref.loss(reg, pos_t, tgt_t, torch.as_tensor(np.asarray(anchors)), iou_loss, iou_metric)
        terms["iou"] = l_iou
        loss, rg = loss + iou_weight * l_iou, rg + iou_weight * l_iou
    if drop != "dir":
        l_dir, _, _ = dir_ref.loss_torch(z_dir, pos_n, tgt_n, anchors, dir_offset)
        terms["dir"] = l_dir
        loss, cls = loss + dir_weight * l_dir, cls + dir_weight * l_dir
    if drop != "iou_head":
        t, _ = iou_head_ref.target_map(reg.detach().numpy(), pos_n, tgt_n, anchors, iou_head_metric)          # a constant
        l_head, out["mae"] = iou_head_ref.loss_torch(z_iou, t, pos_n)
        terms["iou_head"] = l_head
        loss, cls = loss + iou_head_weight * l_head, cls + iou_head_weight * l_head
    out.update(total=loss, loss=loss, cls_loss=cls, reg_loss=rg, cls_pos=cls_pos, cls_neg=cls_neg, terms=terms)
    return out


def tiny_batch(golden):
    """the tiny golden batch (middle_tiny_car + rpn3d_tiny: 10 x 16 x 24 grid, B = 2, 8 x 12 maps, 17 + 16 positives)
    -> (feats, coords: lists of CPU tensors; targets = (pos, neg, targets) float32 arrays)"""
    g, t = golden("middle_tiny_car"), golden("rpn3d_tiny")
    lens = [int(x) for x in g["feat_lens"]]
    feats = list(torch.split(torch.from_numpy(g["features"]), lens))
    coords = list(torch.split(torch.from_numpy(g["coords"]), lens))
    return feats, coords, tuple(np.ascontiguousarray(t[k], dtype=np.float32) for k in ("pos", "neg", "targets"))


def oracle_run(feats, coords, head_params, masks=None, cls_name="Car", dims=TINY_DIMS):
    """The float64 train-mode oracle with both site heads: tr.feature_net -> tr.middle_rpn(taps=, masks=), the concatenation
    as cat([deconv3, deconv2, deconv1]) and a float64 1x1 convolution per head.  head_params: HEAD_KEYS -> tensor (the golden
    state dict has no heads).  masks: test_gpu_model._hip_masks' ReLU decisions, or None for F.relu.
    -> (prob, reg, dir_logits, iou_logits (B,2,h,w) with the autograd graph, leaves: name -> leaf, all 108 of them)"""
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in tr.make_state_dict(cls_name).items()}
    for k in HEAD_KEYS:
        sd[k] = head_params[k].detach().cpu().double()
    keys = tr.param_keys(sd)
    assert len(keys) == 108 and all(k in keys for k in HEAD_KEYS)
    leaves = {k: sd[k].detach().clone().requires_grad_(True) for k in keys}
    work = dict(sd)
    work.update(leaves)
    taps = {}
    dense = tr.feature_net([f.double() for f in feats], coords, work, dims, True)
    prob, reg = tr.middle_rpn(dense, work, cls_name, True, taps=taps, masks=masks)
    cat = torch.cat([taps["deconv3"], taps["deconv2"], taps["deconv1"]], dim=1)
    dir_logits = F.conv2d(cat, leaves[HEAD_KEYS[0]], leaves[HEAD_KEYS[1]])
    iou_logits = F.conv2d(cat, leaves[HEAD_KEYS[2]], leaves[HEAD_KEYS[3]])
    return prob, reg, dir_logits, iou_logits, leaves
