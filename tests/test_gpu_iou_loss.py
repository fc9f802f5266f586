"""GPU: the rotated-IoU regression loss (vn_rpn_iou_loss: csrc/iou_loss.hip) against tests/iou_loss_ref.py in
float64 on the CPU, against the project's own rotated IoU (vn_box_iou_rotated), at planted edge cases, against itself
(run to run, forward-only, a side stream) and through RPN3D (loss, forward, train_step, a short training run).

Bars: the loss kernel's own (tests/test_gpu_loss.py) — 1e-5 relative on the two scalars, 1e-5 of the gradient's maximum on
d_delta; see BARS below for the measured values.

Shapes: the loss tests' own — (3,7,5) = 105 sites, one partial workgroup, no positive in the last sample (P_b clamps to 1);
(2,16,24) = 768 sites, exactly three workgroups; (2,17,15) = 510 sites, two workgroups, the second partial, the sample
boundary (site 255) inside the first; and the two seam shapes of iou_loss_ref.SEAM_CASES, (1,33,63) and (2,129,255), with
a handful of planted positives.  Anchors: iou_loss_ref.small_anchors, a small Car-style grid."""
import functools
import math
from dataclasses import replace

import numpy as np
import pytest
import torch

import focal_ref
import iou_loss_ref as R
from oracle import torch_ref as tr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(3, 7, 5, True), (2, 16, 24, False), (2, 17, 15, False)]
COMBOS = [(k, m) for k in ("iou", "diou") for m in ("bev", "3d")]
UPSTREAM = 0.37
TAIL = 64          # sentinel elements behind d_delta, sentinel bytes behind the workspace
# relative bars (scalars, gradient / gradient maximum): the loss kernel's own.  Measured worst over the three shapes, the four
# (kind, metric) combinations and both upstream choices, MI355X: scalars 4.5e-8, gradient 4.8e-8 of its maximum (the
# arithmetic is float64 up to the fp32 rounding of the outputs); the forward against vn_box_iou_rotated 4.5e-8 (bar 1e-6);
# the heads' regression weight gradient through the module 0 (bf16) and 1.1e-7 (fp32) of its maximum.
BARS = (1e-5, 1e-5)


def _ids(s):
    return "x".join(str(v) for v in s[:3]) if isinstance(s[0], int) else "-".join(s)


@functools.lru_cache(maxsize=None)
def _inputs(shape):
    B, H, W, empty = shape
    delta, pos, tgt = R.generic_inputs(B, H, W, 7 + B, empty)
    return delta, pos, tgt, torch.from_numpy(R.small_anchors(H, W).reshape(-1, 7).copy())


@functools.lru_cache(maxsize=None)
def _reference(shape, kind, metric):
    """float64 iou_loss_ref on the CPU, once per (shape, kind, metric): (loss, mean_iou, d_delta for upstream 1, pairs)"""
    delta, pos, tgt, anchors = _inputs(shape)
    d64 = delta.double().requires_grad_(True)
    loss, mean_iou, pairs = R.loss(d64, pos, tgt, anchors, kind, metric)
    if loss.requires_grad:
        loss.backward()
    grad = d64.grad if d64.grad is not None else torch.zeros_like(d64)
    return loss.item(), mean_iou.item(), grad, pairs


def _launch(delta, pos, tgt, anchors, kind, metric, g=None, forward_only=False, fill=float("nan")):
    """vn_rpn_iou_loss on device tensors -> (out2, d_delta with its TAIL sentinels or None, workspace with its TAIL bytes)"""
    from voxelnet_amd import _lib
    from voxelnet_amd import iou_loss as IL
    B, _, H, W = delta.shape
    wsb = _lib.load().vn_rpn_iou_loss_workspace_bytes(B, H, W)
    ws = torch.full((wsb + TAIL,), 0xA5, dtype=torch.uint8, device=DEV)
    out = torch.full((2,), float("nan"), device=DEV)
    dd = None if forward_only else torch.full((delta.numel() + TAIL,), fill, device=DEV)
    gt = None if g is None else torch.tensor([g], dtype=torch.float32, device=DEV)
    _lib.call("vn_rpn_iou_loss", delta.data_ptr(), pos.data_ptr(), tgt.data_ptr(), anchors.data_ptr(), B, H, W, IL.KINDS[kind],
              IL.METRICS[metric], None if gt is None else gt.data_ptr(), ws.data_ptr(), wsb, out.data_ptr(),
              None if dd is None else dd.data_ptr(), _lib.raw_stream())
    return out, dd, ws


def _grad_of(dd, delta):
    return dd[:delta.numel()].view_as(delta)


def _dev(ts):
    return tuple(t.to(DEV).contiguous() for t in ts)


@pytest.mark.parametrize("combo", COMBOS, ids=_ids)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_scalars_and_gradient_against_the_reference(shape, combo):
    kind, metric = combo
    ins = _dev(_inputs(shape))
    ref_loss, ref_iou, ref_grad, pairs = _reference(shape, kind, metric)
    assert len(pairs) > 10 and all(p[1] > 0.0 for p in pairs)          # every generic pair overlaps: none is left out
    assert math.isfinite(ref_loss) and ref_grad.abs().max().item() > 0
    for g in (None, UPSTREAM):
        out, dd, ws = _launch(*ins, kind, metric, g=g)
        torch.cuda.synchronize()
        got = out.cpu().double().numpy()
        es = max(abs(got[0] - ref_loss) / abs(ref_loss), abs(got[1] - ref_iou) / abs(ref_iou))
        want = ref_grad * (1.0 if g is None else float(np.float32(g)))
        eg = (_grad_of(dd, ins[0]).cpu().double() - want).abs().max().item() / want.abs().max().item()
        print(f"{shape[:3]} {kind} {metric} g={g}: scalars {es:.2e}, gradient {eg:.2e} of the maximum")
        assert torch.isfinite(out).all() and torch.isfinite(dd[:ins[0].numel()]).all()
        assert es <= BARS[0], (got, ref_loss, ref_iou)
        assert eg <= BARS[1]
        assert torch.isnan(dd[ins[0].numel():]).all() and bool((ws[-TAIL:] == 0xA5).all())


@functools.lru_cache(maxsize=None)
def _seam_reference(shape, kind, metric):
    delta, pos, tgt, anchors = R.seam_inputs(shape)
    d64 = delta.double().requires_grad_(True)
    loss, mean_iou, pairs = R.loss(d64, pos, tgt, anchors, kind, metric)
    loss.backward()
    return loss.item(), mean_iou.item(), d64.grad, pairs


@pytest.mark.parametrize("combo", [("iou", "bev"), ("diou", "3d")], ids=_ids)
@pytest.mark.parametrize("shape", list(R.SEAM_CASES), ids=_ids)
def test_seams_of_the_site_term_scaffold(shape, combo):
    """the two loops of csrc/rpn_common.h's scaffold that no shape above reaches (iou_loss_ref.SEAM_CASES, guarded on the
    CPU by tests/test_iou_loss_host.py): k_pos_norm's second sweep over a sample, and k_site_term_finalize's second slab row
    per thread with a workgroup that straddles two samples.  Forward-only and forward + backward, the bars and the sentinel
    tails of test_scalars_and_gradient_against_the_reference."""
    kind, metric = combo
    ins = _dev(R.seam_inputs(shape))
    ref_loss, ref_iou, ref_grad, pairs = _seam_reference(shape, kind, metric)
    assert len(pairs) == len(R.SEAM_CASES[shape]) and all(p[1] > 0.0 for p in pairs)
    assert math.isfinite(ref_loss) and ref_grad.abs().max().item() > 0
    n = ins[0].numel()
    for forward_only in (True, False):
        out, dd, ws = _launch(*ins, kind, metric, forward_only=forward_only)
        torch.cuda.synchronize()
        got = out.cpu().double().numpy()
        es = max(abs(got[0] - ref_loss) / abs(ref_loss), abs(got[1] - ref_iou) / abs(ref_iou))
        print(f"{shape} {kind} {metric} forward_only={forward_only}: scalars {es:.2e} (loss {got[0]:.7f} vs {ref_loss:.7f})")
        assert torch.isfinite(out).all() and es <= BARS[0], (got, ref_loss, ref_iou)
        assert bool((ws[-TAIL:] == 0xA5).all())
        if not forward_only:
            eg = (_grad_of(dd, ins[0]).cpu().double() - ref_grad).abs().max().item() / ref_grad.abs().max().item()
            print(f"{shape} {kind} {metric}: gradient {eg:.2e} of the maximum")
            assert torch.isfinite(dd[:n]).all() and eg <= BARS[1]
            assert torch.isnan(dd[n:]).all()


def _decode_np(d, A):
    d, A = np.asarray(d, dtype=np.float64), np.asarray(A, dtype=np.float64)
    diag = np.sqrt(A[:, 4] ** 2 + A[:, 5] ** 2)
    return np.stack([d[:, 0] * diag + A[:, 0], d[:, 1] * diag + A[:, 1], d[:, 2] * A[:, 3] + A[:, 2], np.exp(d[:, 3]) * A[:, 3],
                     np.exp(d[:, 4]) * A[:, 4], np.exp(d[:, 5]) * A[:, 5], d[:, 6] + A[:, 6]], axis=1)


@pytest.mark.parametrize("metric", ["bev", "3d"])
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_forward_against_the_projects_own_iou(shape, metric):
    """mean_iou and the 1 - IoU terms of the loss from vn_box_iou_rotated on boxes decoded in float64 on the host: only the
    fp32 rounding of out2 separates the two"""
    from voxelnet_amd import _lib
    from voxelnet_amd import iou_loss as IL
    delta, pos, tgt, anchors = _inputs(shape)
    B, H, W = shape[:3]
    idx = torch.nonzero(pos).tolist()
    A = np.stack([anchors.numpy().reshape(H, W, 2, 7)[y, x, a] for _, y, x, a in idx])
    P = _decode_np(np.stack([delta[b, a * 7:a * 7 + 7, y, x].numpy() for b, y, x, a in idx]), A)
    G = _decode_np(np.stack([tgt[b, y, x, a * 7:a * 7 + 7].numpy() for b, y, x, a in idx]), A)
    n = len(idx)
    pd, gd = torch.from_numpy(P).to(DEV), torch.from_numpy(G).to(DEV)
    table = torch.empty((n, n), dtype=torch.float64, device=DEV)
    _lib.call("vn_box_iou_rotated", pd.data_ptr(), n, gd.data_ptr(), n, IL.METRICS[metric], table.data_ptr(), _lib.raw_stream())
    iou = table.diagonal().cpu().numpy()
    p_b = np.maximum(pos.sum(dim=(1, 2, 3)).numpy().astype(np.float64), 1.0)
    want_loss = sum((1.0 - v) / p_b[b] for v, (b, _, _, _) in zip(iou, idx))
    out, _, _ = _launch(*_dev((delta, pos, tgt, anchors)), "iou", metric, forward_only=True)
    got = out.cpu().double().numpy()
    e = max(abs(got[0] - want_loss) / want_loss, abs(got[1] - iou.mean()) / iou.mean())
    print(f"{shape[:3]} {metric}: {e:.2e}")
    assert iou.min() > 0 and e <= 1e-6, (got, want_loss, iou.mean())


# ---- planted edge cases inside (2,16,24): (b, y, x, a) -> (delta, target) of that anchor; every other anchor is a negative
_T = [0.05, -0.02, 0.01, 0.02, -0.03, 0.04, 0.1]          # the target the planted predictions are measured against
INF, NAN = float("inf"), float("nan")
PLANTED = {
    "equal": ((0, 2, 3, 0), _T, _T),                                                   # P == G
    "far": ((0, 5, 20, 1), [7.0, 0.1, 0.0, 0.1, -0.1, 0.05, 0.3], _T),                 # 7 * 4.2 m = 30 m apart
    "p_in_g": ((0, 9, 7, 0), [0.02, 0.01, 0.1, -0.4, -0.5, -0.6, 0.2], _T),
    "g_in_p": ((1, 0, 0, 1), [0.02, 0.01, -0.1, 0.4, 0.5, 0.6, 0.2], _T),
    "no_z": ((1, 15, 23, 0), [0.02, 0.01, 2.0, 0.0, 0.1, 0.1, 0.2], _T),              # footprints overlap, 3.1 m above
    "inf": ((1, 7, 11, 1), [0.0, 0.0, 0.0, INF, 0.0, 0.0, 0.0], _T),
    "nan": ((0, 12, 1, 1), [NAN, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0], _T),
    "huge": ((1, 3, 17, 0), [0.0, 0.0, 0.0, 0.0, 1000.0, 0.0, 0.0], _T),
}
INVALID = ("inf", "nan", "huge")


def _planted(names):
    B, H, W = 2, 16, 24
    g = torch.Generator().manual_seed(99)
    delta = (torch.randn((B, 14, H, W), generator=g) * 0.2).float()
    tgt = (torch.rand((B, H, W, 14), generator=g) * 0.6 - 0.3).float()
    pos = torch.zeros((B, H, W, 2))
    for n in names:
        (b, y, x, a), d, t = PLANTED[n]
        pos[b, y, x, a] = 1.0
        delta[b, a * 7:a * 7 + 7, y, x] = torch.tensor(d)
        tgt[b, y, x, a * 7:a * 7 + 7] = torch.tensor(t)
    return delta, pos, tgt, torch.from_numpy(R.small_anchors(H, W).reshape(-1, 7).copy())


def _slot(name):
    (b, y, x, a), _, _ = PLANTED[name]
    return b, slice(a * 7, a * 7 + 7), y, x


@pytest.mark.parametrize("combo", COMBOS, ids=_ids)
def test_planted_edge_cases(combo):
    kind, metric = combo
    # each case alone: out2 = [L, IoU] of that pair
    alone = {}
    for name in PLANTED:
        ins = _dev(_planted([name]))
        out, dd, _ = _launch(*ins, kind, metric)
        grad = _grad_of(dd, ins[0]).cpu()
        assert torch.isfinite(out).all() and torch.isfinite(grad).all(), name
        alone[name] = (out[0].item(), out[1].item(), grad[_slot(name)].clone())
        grad[_slot(name)] = 0.0
        assert grad.abs().max().item() == 0.0 and not torch.signbit(grad).any(), name          # zeros wherever pos == 0
    L, iou, g = alone["equal"]
    assert abs(iou - 1.0) <= 1e-6 and abs(L) <= 1e-6
    for name in INVALID:
        L, iou, g = alone[name]
        assert (L, iou) == (1.0, 0.0) and g.abs().max().item() == 0.0, name
    disjoint = ("far", "no_z") if metric == "3d" else ("far",)
    for name in disjoint:
        L, iou, g = alone[name]
        assert iou == 0.0, name
        if kind == "iou":
            assert L == 1.0 and g.abs().max().item() == 0.0, name
        else:
            assert L > 1.0 and g.abs().max().item() > 0.0, name
    assert 0.0 < alone["p_in_g"][1] < 1.0 and 0.0 < alone["g_in_p"][1] < 1.0
    # all of them together, d_delta pre-filled with NaN, against the reference; the gradient at P == G — a point where IoU
    # is not smooth — only has to be finite
    cpu = _planted(list(PLANTED))
    d64 = cpu[0].double().requires_grad_(True)
    ref_loss, ref_iou, pairs = R.loss(d64, cpu[1], cpu[2], cpu[3], kind, metric)
    ref_loss.backward()
    want = d64.grad.clone()
    ins = _dev(cpu)
    out, dd, ws = _launch(*ins, kind, metric)
    got = _grad_of(dd, ins[0]).cpu().double()
    assert torch.isfinite(out).all() and torch.isfinite(got).all()
    assert bool((got[cpu[1].repeat_interleave(7, dim=3).permute(0, 3, 1, 2) == 0] == 0.0).all())
    assert torch.isnan(dd[ins[0].numel():]).all() and bool((ws[-TAIL:] == 0xA5).all())
    got[_slot("equal")] = 0.0
    want[_slot("equal")] = 0.0
    o = out.cpu().double().numpy()
    assert abs(o[0] - ref_loss.item()) <= BARS[0] * abs(ref_loss.item()) and abs(o[1] - ref_iou.item()) <= BARS[0] * ref_iou.item()
    assert want.abs().max().item() > 0 and (got - want).abs().max().item() <= BARS[1] * want.abs().max().item()
    for name in ("p_in_g", "g_in_p") + (("far",) if kind == "diou" else ()):
        assert want[_slot(name)].abs().max().item() > 0, name          # (these cases carry a gradient the comparison saw)


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_determinism_and_forms(shape):
    """two runs bit-identical; the forward-only call gives the same out2; a side stream gives the same bits"""
    ins = _dev(_inputs(shape))
    for kind, metric in COMBOS:
        out_a, dd_a, ws_a = _launch(*ins, kind, metric, g=UPSTREAM)
        out_b, dd_b, ws_b = _launch(*ins, kind, metric, g=UPSTREAM, fill=0.0)
        out_f, _, _ = _launch(*ins, kind, metric, forward_only=True)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            out_s, dd_s, ws_s = _launch(*ins, kind, metric, g=UPSTREAM)
        torch.cuda.synchronize()
        n = ins[0].numel()
        assert torch.equal(out_a, out_b) and torch.equal(dd_a[:n], dd_b[:n]) and torch.equal(ws_a, ws_b)
        assert torch.equal(out_a, out_f)
        assert torch.equal(out_a, out_s) and torch.equal(dd_a[:n], dd_s[:n]) and torch.equal(ws_a, ws_s)
        assert torch.isfinite(out_a).all()


def test_autograd_function_scales_by_the_upstream_gradient():
    """iou_loss.rpn_iou_loss: (loss, mean_iou) of the raw call, d(2.5 * loss)/d delta = 2.5 * d_delta, no graph under no_grad"""
    from voxelnet_amd import iou_loss as IL
    delta, pos, tgt, anchors = _dev(_inputs(SHAPES[2]))
    out, dd, _ = _launch(delta, pos, tgt, anchors, "diou", "3d")
    d = delta.clone().requires_grad_(True)
    loss, mean_iou = IL.rpn_iou_loss(d, pos, tgt, anchors.view(17, 15, 2, 7), "diou", "3d")
    assert loss.requires_grad and not mean_iou.requires_grad
    (2.5 * loss).backward()
    assert torch.equal(torch.stack([loss.detach(), mean_iou]), out)
    assert torch.equal(d.grad, _grad_of(dd, delta) * 2.5)
    with torch.no_grad():
        l2, m2 = IL.rpn_iou_loss(d, pos, tgt, anchors, "diou", "3d")
    assert not l2.requires_grad and torch.equal(l2, loss.detach()) and torch.equal(m2, mean_iou)


# ---- through the module, on the tiny golden batch (tests/golden/middle_tiny_car.npz + rpn3d_tiny.npz: 10 x 16 x 24 grid,
# B = 2, 8 x 12 maps, 17 + 16 positive anchors).  The IoU term takes its anchors from the module's target generator; the
# tiny maps get a generator with an 8 x 12 grid of the small anchors (the Car generator's grid is the full 200 x 176 one).
ABS = (1.5, 1.0, 3.0)
DIOU = dict(iou_loss="diou", iou_weight=2.0)
FOCAL = dict(cls_loss="focal", focal_alpha=0.25, focal_gamma=2.0, yaw_loss="sin")


def _tiny(golden):
    g, t = golden("middle_tiny_car"), golden("rpn3d_tiny")
    lens = [int(x) for x in g["feat_lens"]]
    feats = list(torch.split(torch.from_numpy(g["features"]), lens))
    coords = list(torch.split(torch.from_numpy(g["coords"]), lens))
    targets = tuple(np.ascontiguousarray(t[k], dtype=np.float32) for k in ("pos", "neg", "targets"))
    batch = (None, None, [f.to(DEV) for f in feats], None, [c.to(DEV) for c in coords], None, None)
    return batch, targets


def _tiny_model(mode, **kw):
    from voxelnet_amd import model as M
    from voxelnet_amd.targets import TargetGenerator
    M.set_precision(mode)
    m = M.RPN3D("Car", **kw)
    m.load_state_dict(tr.make_state_dict("Car"))
    m.feature_net._grid = replace(m.feature_net._grid, H=16, W=24)
    m = m.to(DEV).train()
    m.__dict__["_targets"] = TargetGenerator("Car", DEV, anchors=R.small_anchors(8, 12))
    return m


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_module_without_the_term_is_what_it_was(golden, mode):
    """RPN3D(iou_loss=None, ...): forward and train_step bit-identical to a model built without the arguments, and still
    the one-call step"""
    from voxelnet_amd import model as M
    batch, targets = _tiny(golden)
    try:
        res = []
        for kw in ({}, dict(iou_loss=None, iou_weight=3.0, iou_metric="bev")):
            m = _tiny_model(mode, **kw)
            fwd = m(batch, DEV, targets=targets)
            m2 = _tiny_model(mode, **kw)
            assert m2._step_fused_ok(mode, None)
            step = m2.train_step(batch, DEV, None, targets=targets)
            torch.cuda.synchronize()
            assert m.last_iou is None and m2.last_iou is None
            res.append((fwd, step, [p.grad for p in m2.parameters()]))
    finally:
        M.set_precision("bf16")
    (fa, sa, ga), (fb, sb, gb) = res
    assert all(torch.equal(x, y) for x, y in zip(fa, fb)) and all(torch.equal(x, y) for x, y in zip(sa, sb))
    assert all(x is not None and torch.equal(x, y) for x, y in zip(ga, gb))


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_module_with_the_diou_term(golden, mode):
    """iou_loss="diou", iou_weight=2: the loss is the base loss + 2 * rpn_iou_loss on the same maps, in bits; train_step
    equals forward + backward + optimizer.step() in every .grad and parameter; the gradient of the heads' regression weight
    equals, at 1e-5 of its maximum, the one the module's backward makes of the float64 references' map gradients
    (focal_ref's loss + 2 * iou_loss_ref's on the module's own maps)"""
    from voxelnet_amd import iou_loss as IL
    from voxelnet_amd import model as M
    from voxelnet_amd.optim import ClipAdamW
    batch, targets = _tiny(golden)
    try:
        a = _tiny_model(mode, **DIOU)
        assert not a._step_fused_ok(mode, None)
        opt_a = ClipAdamW(list(a.parameters()), lr=1e-3, max_norm=5.0)
        before = [p.detach().clone() for p in a.parameters()]
        out_a = a.train_step(batch, DEV, opt_a, targets=targets)
        b = _tiny_model(mode, **DIOU)
        opt_b = ClipAdamW(list(b.parameters()), lr=1e-3, max_norm=5.0)
        out_b = b(batch, DEV, targets=targets)
        out_b[2].backward()
        grads_b = [p.grad.detach().clone() for p in b.parameters()]
        opt_b.step()
        c = _tiny_model(mode)
        out_c = c(batch, DEV, targets=targets)
        # the references' map gradients through the module's own backward
        d = _tiny_model(mode)
        out_d = d(batch, DEV, targets=targets)
        pos, neg, tgt = (torch.from_numpy(t) for t in targets)
        p64 = out_d[0].detach().cpu().double().requires_grad_(True)
        d64 = out_d[1].detach().cpu().double().requires_grad_(True)
        anchors = torch.from_numpy(R.small_anchors(8, 12).reshape(-1, 7).copy())
        ref = focal_ref.loss(p64, d64, pos.double(), neg.double(), tgt.double(), *ABS, cls="bce")[0] + \
            2.0 * R.loss(d64, pos, tgt, anchors, "diou", "3d")[0]
        ref.backward()
        torch.autograd.backward([out_d[0], out_d[1]], [p64.grad.to(DEV, out_d[0].dtype), d64.grad.to(DEV, out_d[1].dtype)])
        l_iou, mean_iou = IL.rpn_iou_loss(out_c[1].detach(), pos.to(DEV), tgt.to(DEV), anchors.to(DEV), "diou", "3d")
        torch.cuda.synchronize()
    finally:
        M.set_precision("bf16")
    assert len(out_a) == len(out_b) == 7
    for i, (x, y) in enumerate(zip(out_a, out_b)):
        assert torch.isfinite(x).all() and torch.equal(x, y), (mode, "output", i)
    assert torch.equal(out_b[0], out_c[0]) and torch.equal(out_b[1], out_c[1])          # the same maps
    assert torch.equal(out_b[2], out_c[2] + 2.0 * l_iou) and torch.equal(out_b[4], out_c[4] + 2.0 * l_iou)
    assert all(torch.equal(out_b[i], out_c[i]) for i in (3, 5, 6))
    assert torch.equal(b.last_iou[0], l_iou) and torch.equal(b.last_iou[1], mean_iou) and not b.last_iou[0].requires_grad
    assert l_iou.item() > 0 and out_b[2].item() != out_c[2].item()
    for (k, pa), pb, gb, p0 in zip(a.named_parameters(), b.parameters(), grads_b, before):
        assert pa.grad is not None and torch.isfinite(pa.grad).all() and torch.equal(pa.grad, gb), (mode, k)
        assert torch.equal(pa.detach(), pb.detach()), (mode, k)
    assert any(not torch.equal(pa.detach(), p0) for pa, p0 in zip(a.parameters(), before))
    got = grads_b[[k for k, _ in b.named_parameters()].index("middle_rpn.reg_conv.conv.weight")].double()
    want = dict(d.named_parameters())["middle_rpn.reg_conv.conv.weight"].grad.double()
    e = (got - want).abs().max().item() / want.abs().max().item()
    print(f"{mode}: heads' regression weight gradient {e:.2e} of its maximum")
    assert want.abs().max().item() > 0 and e <= 1e-5


def test_ten_adamw_steps_with_focal_sine_and_diou(golden):
    """ten ClipAdamW steps (lr 1e-3) on the tiny batch with focal + sine + diou: the IoU term ends below its first value,
    everything stays finite"""
    from voxelnet_amd import model as M
    from voxelnet_amd.optim import ClipAdamW
    batch, targets = _tiny(golden)
    try:
        m = _tiny_model("bf16", **FOCAL, iou_loss="diou")
        opt = ClipAdamW(list(m.parameters()), lr=1e-3, max_norm=5.0)
        terms, losses = [], []
        for _ in range(10):
            out = m.train_step(batch, DEV, opt, targets=targets)
            terms.append(m.last_iou)
            losses.append(out[2])
            opt.zero_grad(set_to_none=True)
        terms = [(float(l), float(i)) for l, i in terms]
        losses = [float(x) for x in losses]
    finally:
        M.set_precision("bf16")
    print("focal + sine + diou, ten ClipAdamW steps: L_iou", " ".join(f"{l:.4f}" for l, _ in terms),
          "| mean IoU", " ".join(f"{i:.4f}" for _, i in terms))
    assert all(np.isfinite(losses)) and all(np.isfinite(t).all() for t in terms)
    assert terms[-1][0] < terms[0][0], terms
    assert all(torch.isfinite(p).all() for p in m.parameters())
