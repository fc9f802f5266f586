"""Float64 restatement of the rotated-IoU regression loss in torch ops with autograd — the reference
tests/test_iou_loss_host.py checks against tests/eval_ref.py and tests/test_gpu_iou_loss.py holds csrc/iou_loss.hip against.
Sutherland-Hodgman on torch scalars, one Python loop per positive anchor; no derivative is written out anywhere here, and
nothing is shared with the library (voxelnet_amd is not imported).

Box = (x, y, z, h, w, l, r): footprint corners (+-l/2, +-w/2) turned by r about (x, y); vertical extent [z, z + h]."""
import math

import torch

F64 = torch.float64


def _f(v):
    return v.detach().item()


def decode(d, A):
    """seven regression values d and the anchor A (x, y, z, h, w, l, r) -> the box, as torch float64 scalars"""
    diag = torch.sqrt(A[4] * A[4] + A[5] * A[5])
    return [d[0] * diag + A[0], d[1] * diag + A[1], d[2] * A[3] + A[2], torch.exp(d[3]) * A[3], torch.exp(d[4]) * A[4],
            torch.exp(d[5]) * A[5], d[6] + A[6]]


def _corners(l, w, r, cx, cy):
    c, s = torch.cos(r), torch.sin(r)
    return [(sx * l / 2 * c - sy * w / 2 * s + cx, sx * l / 2 * s + sy * w / 2 * c + cy)
            for sx, sy in ((1, 1), (-1, 1), (-1, -1), (1, -1))]          # counter-clockwise


def _clip(poly, e0, e1):
    """the part of `poly` on the left of the directed line e0 -> e1"""
    dx, dy = e1[0] - e0[0], e1[1] - e0[1]
    out = []
    for i, cur in enumerate(poly):
        prev = poly[i - 1]
        dp = dx * (prev[1] - e0[1]) - dy * (prev[0] - e0[0])
        dc = dx * (cur[1] - e0[1]) - dy * (cur[0] - e0[0])
        if (dp.item() >= 0) != (dc.item() >= 0):
            t = dp / (dp - dc)
            out.append((prev[0] + (cur[0] - prev[0]) * t, prev[1] + (cur[1] - prev[1]) * t))
        if dc.item() >= 0:
            out.append(cur)
    return out


def bev_intersection(P, G):
    """area of the two footprints' intersection (torch scalar); P's centre is the origin of the computation"""
    zero = torch.zeros((), dtype=F64)
    poly = _corners(P[5], P[4], P[6], zero, zero)
    pg = _corners(G[5], G[4], G[6], G[0] - P[0], G[1] - P[1])
    for k in range(4):
        poly = _clip(poly, pg[k], pg[(k + 1) % 4])
        if not poly:
            return zero
    s = zero
    for i, p in enumerate(poly):
        q = poly[(i + 1) % len(poly)]
        s = s + (p[0] * q[1] - q[0] * p[1])
    return 0.5 * torch.abs(s)


def _valid(P, G, metric):
    vals = [_f(v) for v in P + G]
    if not all(math.isfinite(v) for v in vals) or min(vals[3:6] + vals[10:13]) <= 0:
        return False
    den = vals[4] * vals[5] + vals[11] * vals[12] if metric == "bev" else \
        vals[3] * vals[4] * vals[5] + vals[10] * vals[11] * vals[12]
    return math.isfinite(den) and den > 0


def distance_term(P, G, metric):
    """rho2 / c2 of the DIoU form (torch scalar), None where the term is skipped"""
    pts = _corners(P[5], P[4], P[6], P[0], P[1]) + _corners(G[5], G[4], G[6], G[0], G[1])
    xs, ys = torch.stack([p[0] for p in pts]), torch.stack([p[1] for p in pts])
    ex, ey = xs.max() - xs.min(), ys.max() - ys.min()
    rho2 = (G[0] - P[0]) ** 2 + (G[1] - P[1]) ** 2
    c2 = ex ** 2 + ey ** 2
    if metric == "3d":
        rho2 = rho2 + ((G[2] + G[3] / 2) - (P[2] + P[3] / 2)) ** 2
        ez = torch.maximum(P[2] + P[3], G[2] + G[3]) - torch.minimum(P[2], G[2])
        c2 = c2 + ez ** 2
    if not (math.isfinite(_f(rho2)) and math.isfinite(_f(c2)) and _f(c2) > 0):
        return None
    return rho2 / c2


def pair_loss(P, G, kind, metric):
    """-> (IoU, L) torch scalars of one decoded pair; an invalid pair gives the constants (0, 1)"""
    if not _valid(P, G, metric):
        return torch.zeros((), dtype=F64), torch.ones((), dtype=F64)
    inter = bev_intersection(P, G)
    if metric == "bev":
        den = P[4] * P[5] + G[4] * G[5] - inter
        iou = inter / den
    else:
        zo = torch.clamp(torch.minimum(P[2] + P[3], G[2] + G[3]) - torch.maximum(P[2], G[2]), min=0.0)
        inter3 = inter * zo
        den = P[3] * P[4] * P[5] + G[3] * G[4] * G[5] - inter3
        iou = inter3 / den
    if not _f(den) > 0:
        return torch.zeros((), dtype=F64), torch.ones((), dtype=F64)
    L = 1.0 - iou
    if kind == "diou":
        d = distance_term(P, G, metric)
        if d is not None:
            L = L + d
    return iou, L


def loss(delta, pos, targets, anchors, kind="iou", metric="3d"):
    """delta (B,14,H,W), pos (B,H,W,2), targets (B,H,W,14), anchors (H*W*2,7) or (H,W,2,7): torch tensors, widened to
    float64 here (delta may require grad) -> (loss, mean_iou, pairs) with pairs = [((b, y, x, a), IoU, L)] of the anchors
    with pos != 0 in index order"""
    assert kind in ("iou", "diou") and metric in ("bev", "3d")
    delta, pos, targets = delta.to(F64), pos.to(F64), targets.to(F64)
    B, _, H, W = delta.shape
    anchors = torch.as_tensor(anchors, dtype=F64).reshape(H, W, 2, 7)
    p_b = pos.sum(dim=(1, 2, 3)).clamp(min=1.0)
    total = torch.zeros((), dtype=F64)
    s_iou = torch.zeros((), dtype=F64)
    pairs = []
    for b, y, x, a in torch.nonzero(pos).tolist():
        A = anchors[y, x, a]
        m = pos[b, y, x, a]
        P = decode(delta[b, a * 7:a * 7 + 7, y, x], A)
        G = decode(targets[b, y, x, a * 7:a * 7 + 7].detach(), A)
        iou, L = pair_loss(P, G, kind, metric)
        total = total + m * L / p_b[b]
        s_iou = s_iou + m * iou.detach()
        pairs.append(((b, y, x, a), _f(iou), _f(L)))
    return total, s_iou / pos.sum().clamp(min=1.0), pairs


# ---------------------------------------------------------------------------------------------------- test inputs
def small_anchors(H, W):
    """a small Car-style anchor grid (H, W, 2, 7) float64: centres on a linspace over the Car range, yaws 0 and pi/2"""
    import numpy as np
    gx, gy = np.meshgrid(np.linspace(0.0, 70.4, W), np.linspace(-40.0, 40.0, H))
    a = np.empty((H, W, 2, 7))
    a[..., 0], a[..., 1] = gx[..., None], gy[..., None]
    a[..., 2], a[..., 3], a[..., 4], a[..., 5] = -1.0, 1.56, 1.6, 3.9
    a[..., 0, 6], a[..., 1, 6] = 0.0, np.pi / 2
    return a


def generic_inputs(B, H, W, seed, empty_last=False, flat=None):
    """-> delta (B,14,H,W), pos (B,H,W,2), targets (B,H,W,14) float32: pos Bernoulli 0.1, targets uniform in +-0.3, delta at
    the positives = target + uniform +-0.2 (yaw +-0.5), randn * 0.2 elsewhere.  empty_last: no positive in the last sample;
    flat: the positives are exactly these flat elements of pos (2 * global site + rotation) instead"""
    g = torch.Generator().manual_seed(seed)
    pos = (torch.rand((B, H, W, 2), generator=g) < 0.1).float()
    if empty_last:
        pos[-1] = 0
    if flat is not None:
        pos = torch.zeros(B * H * W * 2)
        pos[list(flat)] = 1.0
        pos = pos.view(B, H, W, 2)
    tgt = (torch.rand((B, H, W, 14), generator=g) * 0.6 - 0.3).float()
    noise = torch.rand((B, H, W, 14), generator=g) * 0.4 - 0.2
    noise[..., 6::7] = torch.rand((B, H, W, 2), generator=g) * 1.0 - 0.5
    near = (tgt + noise).permute(0, 3, 1, 2)
    far = torch.randn((B, 14, H, W), generator=g) * 0.2
    mask = pos.repeat_interleave(7, dim=3).permute(0, 3, 1, 2) != 0
    delta = torch.where(mask, near, far).float().contiguous()
    return delta, pos, tgt


# The two loops of the site-term scaffold (csrc/rpn_common.h) that no shape of <= 768 sites reaches, as (B, H, W) -> the
# flat elements of pos that are positive.
# (1,33,63): 2,079 sites, 4,158 elements of pos > 16 x 256, so k_pos_norm's loop takes a second, partial sweep: elements
#   4095 / 4096 are the last of the first sweep and the first of the second, 4157 the very last.  P_b = 4; 2 if the second
#   sweep were dropped.
# (2,129,255): 65,790 sites in 257 workgroups, so thread 0 of k_site_term_finalize adds slab rows 0 and 256.  Sites 32,894
#   and 32,895 are the last of sample 0 and the first of sample 1 inside workgroup 128, which therefore sees two values of
#   P_b (4 and 5); sites 255 / 256 and 65,535 / 65,536 straddle workgroups 0 / 1 and 255 / 256; 65,789 is the very last site.
SEAM_CASES = {
    (1, 33, 63): (0, 4095, 4096, 4157),
    (2, 129, 255): (0, 2 * 255, 2 * 256 + 1, 2 * 32894 + 1, 2 * 32895, 2 * 40000, 2 * 65535, 2 * 65536 + 1, 2 * 65789 + 1),
}


def seam_inputs(shape):
    """-> delta, pos, targets (generic_inputs' recipe, the positives exactly SEAM_CASES[shape]) and anchors (H*W*2, 7)"""
    B, H, W = shape
    delta, pos, tgt = generic_inputs(B, H, W, 31 + B, flat=SEAM_CASES[shape])
    return delta, pos, tgt, torch.from_numpy(small_anchors(H, W).reshape(-1, 7).copy())
