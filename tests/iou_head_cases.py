"""Inputs of the IoU-aware confidence head's tests, shared by tests/test_iou_head_host.py — which asserts
the guards on the reference alone (tests/iou_head_ref.py) — and tests/test_gpu_iou_head.py."""
import functools
import math

import numpy as np
import torch

import iou_loss_ref as IR
from oracle import targets as ot

# tests/test_gpu_iou_loss.py's maps: (B, H, W, no positive in the last sample)
LOSS_SHAPES = ((3, 7, 5, True), (2, 16, 24, False), (2, 17, 15, False))
METRICS = ("bev", "3d")
HAND_LOGITS = (0.0, 30.0, -30.0)          # at the first three positives: q = 1/2 and the two saturated branches of log1p(exp(-|z|))
SENTINEL = 777.25
ALPHAS = (0.25, 0.5, 1.0)
RECTIFY_N = (1, 255, 256, 257)
FUSED_M = (1, 63, 64, 65, 129)            # rows: below / at / above one 64-row tile, and a third tile of one row


def _logits(pos, seed):
    """(B,2,H*W) float32: uniform in +-4, HAND_LOGITS at the first positives in the logits' layout"""
    B, H, W, _ = pos.shape
    g = torch.Generator().manual_seed(seed)
    z = (torch.rand((B, 2, H * W), generator=g) * 8.0 - 4.0).float()
    site = pos.reshape(B, H * W, 2).permute(0, 2, 1)
    for (b, a, s), v in zip(torch.nonzero(site).tolist(), HAND_LOGITS):
        z[b, a, s] = v
    return z


@functools.lru_cache(maxsize=None)
def loss_case(shape):
    """-> (logits (B,2,H*W), delta (B,14,H,W), pos (B,H,W,2), targets (B,H,W,14)) float32 and anchors (H*W*2, 7) float64:
    tests/test_gpu_iou_loss.py's generic inputs at this shape"""
    B, H, W, empty = shape
    delta, pos, tgt = IR.generic_inputs(B, H, W, 7 + B, empty)
    return _logits(pos, 41 + H), delta, pos, tgt, torch.from_numpy(IR.small_anchors(H, W).reshape(-1, 7).copy())


@functools.lru_cache(maxsize=None)
def seam_case(shape):
    delta, pos, tgt, anchors = IR.seam_inputs(shape)
    return _logits(pos, 43 + shape[1]), delta, pos, tgt, anchors


def invalid_case():
    """loss_case((2,16,24)) with one planted invalid pair: the first positive's target length channel overflows exp"""
    z, delta, pos, tgt, anchors = loss_case(LOSS_SHAPES[1])
    tgt = tgt.clone()
    b, y, x, a = torch.nonzero(pos)[0].tolist()
    tgt[b, y, x, 7 * a + 5] = 800.0
    return (z, delta, pos, tgt, anchors), (b, a, y * pos.shape[2] + x)


def rectify_case(n, seed=53):
    """-> p, z float32 (n,): p uniform in (0, 1) with 0, 1 and the smallest subnormal planted, z uniform in +-6 with +-30"""
    rng = np.random.default_rng(seed + n)
    p = rng.random(n).astype(np.float32)
    z = (rng.random(n) * 12.0 - 6.0).astype(np.float32)
    for i, v in enumerate((0.0, 1.0, np.float32(1.4e-45))):
        if i < n:
            p[-1 - i] = v
    if n > 8:
        z[0], z[1], z[-1], z[-2] = 30.0, -30.0, 30.0, -30.0          # (also against p = 0 and p = 1)
    else:
        z[0] = 30.0
    return p, z


# ---- the round trip: two overlapping anchors, the worse-placed one more confident ----
RT_SCORE_THRES, RT_NMS_THRES = 0.1, 0.1
RT_SITE_A, RT_SITE_B = 5, 6          # neighbours along x on the (4, 4) grid: 0.4 m apart, rotation 0


def round_trip_anchors():
    return np.ascontiguousarray(ot.generate_anchors("Car")[100:104, 60:64])


def round_trip_maps():
    """-> probs (1,2,4,4), deltas (1,14,4,4), iou_logits (1,2,4,4) float32 in the site layout.  Every delta is 0, so an anchor
    decodes onto itself; the ground truth IS anchor A = (site 5, rotation 0), p = 0.6, q = 0.9; anchor B = (site 6, rotation
    0), the same box 0.4 m further along its length, p = 0.7, q = 0.2; every other anchor has p = 0.01 and z = -30."""
    probs = np.full((1, 2, 16), 0.01, dtype=np.float32)
    z = np.full((1, 2, 16), -30.0, dtype=np.float32)
    probs[0, 0, RT_SITE_A], probs[0, 0, RT_SITE_B] = 0.6, 0.7
    z[0, 0, RT_SITE_A], z[0, 0, RT_SITE_B] = math.log(0.9 / 0.1), math.log(0.2 / 0.8)
    return probs.reshape(1, 2, 4, 4), np.zeros((1, 14, 4, 4), dtype=np.float32), z.reshape(1, 2, 4, 4)


def round_trip_iou_ab():
    """the rotated BEV IoU of anchors A and B: the same (w, l) rectangle shifted by dx along its length"""
    an = round_trip_anchors().reshape(-1, 7)
    A, B = an[2 * RT_SITE_A], an[2 * RT_SITE_B]
    assert A[6] == B[6] == 0.0 and A[1] == B[1]
    dx = abs(B[0] - A[0])
    inter = max(A[5] - dx, 0.0) * A[4]
    return inter / (2 * A[4] * A[5] - inter)
