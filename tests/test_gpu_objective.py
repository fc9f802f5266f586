"""GPU: the full training objective of RPN3D — focal + sine + 2 DIoU + dir_weight L_dir + 1 L_iou_head, both site heads on —
as ONE backward against the float64 composition of the single-term references (tests/objective_ref.py), on the tiny golden
batch (10 x 16 x 24 grid, B = 2, 8 x 12 maps, 33 positives).

With the heads on, training leaves the native executor, and three writers touch the concatenation's gradient in
net._middle_backward: the heads' data gradient writes it, dir_head_backward adds to it in place for the direction head and
again for the IoU-aware head; the regression map receives gradient from the base loss and from the IoU term.  The
single-term tests compare paths that share this backward, or hold the trunk at the 5e-2 a ReLU-mask flip needs, under which a
lost or doubled term stays (tests/test_objective_host.py has the figures).  Here:

  a  all 108 gradients of the public path against the oracle run with the device's own ReLU decisions, at OBJECTIVE_BAR;
  b  the concatenation's gradient across the two in-place accumulations, in bf16 and fp32, against float64 from the device's
     own operands, at the kernel's own bar (one unit in the last place of the stored type);
  c  train_step == forward + backward + step() with everything on, by bits;
  d  all three weights at 0 == the focal + sine model without heads, by bits.

What a fails on is established without the device: tests/test_objective_host.py shows that the reference with any ONE of the
five terms left out moves every trunk and VFE gradient by at least three times OBJECTIVE_BAR."""
from dataclasses import replace

import numpy as np
import pytest
import torch

import dir_ref
import objective_ref as O
from oracle import torch_ref as tr
from test_gpu_dir_head import TDT, _bits, _ordered
from test_gpu_model import _hip_masks, rel_err
from test_objective_host import DIR_WEIGHT, host_head_params

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MAP_BAR = 1e-4          # test_fp32_backward_chain_with_frozen_masks' bar on the maps
SCALAR_BAR = 2e-3       # test_rpn3d_forward_loss' bar on the scalars, which the one-head oracle tests use too
ZERO_BIAS_BAR = 1e-3    # test_detect_fwd_bwd_fp32's absolute bar on a bias in front of a train-mode BatchNorm
FULL = dict(O.MODEL_KW, dir_weight=DIR_WEIGHT)
FOCAL_SINE = {k: FULL[k] for k in ("cls_loss", "focal_alpha", "focal_gamma", "yaw_loss")}


def _tiny(golden):
    feats, coords, targets = O.tiny_batch(golden)
    batch = (["000000", "000001"], None, [f.to(DEV) for f in feats], None, [c.to(DEV) for c in coords], None, None)
    return feats, coords, targets, batch


def _tiny_model(mode, native=True, **kw):
    """test_gpu_iou_head._tiny_model: the golden weights, the heads' own initialisation under seed 7, the 16 x 24 grid, the
    tiny anchors (with the headings kept when the direction head is on)"""
    from voxelnet_amd import model as M
    from voxelnet_amd.targets import TargetGenerator
    M.set_precision(mode)
    torch.manual_seed(7)
    m = M.RPN3D("Car", **kw)
    res = m.load_state_dict(tr.make_state_dict("Car"), strict=False)
    assert all("dir_conv" in k or "iou_conv" in k for k in res.missing_keys) and not res.unexpected_keys
    m.feature_net._grid = replace(m.feature_net._grid, H=16, W=24)
    m.native_executor = native
    m = m.to(DEV).train()
    m.__dict__["_targets"] = TargetGenerator("Car", DEV, anchors=O.ANCHORS_TINY, keep_heading=bool(kw.get("dir_head")))
    return m


def _same(x, y):
    return torch.equal(_bits(x.detach().float()), _bits(y.detach().float()))


# ------------------------------------------------------------------------------------ a. the composed objective, fp32
def test_composed_objective_against_the_frozen_mask_oracle(golden, monkeypatch):
    """fp32, the public path: out = m(batch, DEV, targets=targets); out[2].backward().  A spy around net.middle_forward keeps
    the forward's state, whose stored activations give the ReLU decisions (test_gpu_model._hip_masks); the oracle is
    objective_ref.oracle_run with those masks and objective_ref.objective on its maps and logits, float64, autograd through
    the heads, the trunk and the VFE.

    Bars: maps and both logit maps 1e-4 of the maximum; the five scalars and L_iou, L_dir, L_iou_head 2e-3 relative; every one
    of the 108 gradients within OBJECTIVE_BAR = 5e-4 relative L2 (measured worst: 4.3e-5 at feature_net.vfe_2.bn.weight,
    below a third of the bar, which therefore stays where test_fp32_backward_chain_with_frozen_masks has it; maps and logits
    measured <= 1.9e-5, scalars <= 1.6e-6); a conv / deconv bias in front of a BatchNorm
    below 1e-3 absolute."""
    from voxelnet_amd import model as M
    from voxelnet_amd import net as N
    feats, coords, targets, batch = _tiny(golden)
    states, real = [], N.middle_forward

    def spy(*a, **kw):
        out = real(*a, **kw)
        states.append(out[-1])
        return out
    try:
        m = _tiny_model("fp32", **FULL)
        assert not m._native_ok("fp32")
        monkeypatch.setattr(N, "middle_forward", spy)
        out = m(batch, DEV, targets=targets)
        monkeypatch.setattr(N, "middle_forward", real)
        assert len(states) == 1
        masks = _hip_masks(states[0])
        out[2].backward()
        torch.cuda.synchronize()
    finally:
        M.set_precision("bf16")
    got = dict(m.named_parameters())
    assert len(got) == 108
    heads = {k: got[k].detach().cpu() for k in O.HEAD_KEYS}
    want_heads = host_head_params()
    assert all(torch.equal(heads[k], want_heads[k]) for k in O.HEAD_KEYS)          # the weights the host test judged
    prob, reg, z_dir, z_iou, leaves = O.oracle_run(feats, coords, heads, masks=masks)
    kw = {k: v for k, v in FULL.items() if k not in ("dir_head", "iou_head")}
    ref = O.objective(prob, reg, z_dir, z_iou, *targets, O.ANCHORS_TINY, alpha=float(m.alpha), beta=float(m.beta), sigma=float(m.sigma), **kw)
    ref["total"].backward()
    print("guards:", ref["guards"])
    # maps and logits
    em = {"prob": rel_err(out[0], prob.detach().float().numpy()), "reg": rel_err(out[1], reg.detach().float().numpy()),
          "dir": rel_err(m.last_dir_logits, z_dir.detach().float().numpy()), "iou": rel_err(m.last_iou_logits, z_iou.detach().float().numpy())}
    print("maps vs the frozen-mask oracle:", {k: f"{v:.2e}" for k, v in em.items()})
    assert max(em.values()) < MAP_BAR, em
    # scalars
    dev5 = [float(o.detach()) for o in out[2:7]]
    ref5 = [float(ref[k].detach()) for k in ("loss", "cls_loss", "reg_loss", "cls_pos", "cls_neg")]
    t = {k: float(v.detach()) for k, v in ref["terms"].items()}
    l_iou, l_dir, l_head = float(m.last_iou[0]), float(m.last_dir[0]), float(m.last_iou_head[0])
    print(f"scalars {dev5} vs {ref5}; L_iou {l_iou:.6f} vs {t['iou']:.6f}, L_dir {l_dir:.6f} vs {t['dir']:.6f}, L_iou_head {l_head:.6f} "
          f"vs {t['iou_head']:.6f}")
    np.testing.assert_allclose(dev5, ref5, rtol=SCALAR_BAR)
    np.testing.assert_allclose([l_iou, l_dir, l_head], [t["iou"], t["dir"], t["iou_head"]], rtol=SCALAR_BAR)
    # which scalar each term is added to: every weighted term is far above the scalar bar of the sum it joins (so the
    # comparison above sees a term in the wrong sum), and the device's own sums close at fp32 rounding
    w_iou, w_dir, w_head = kw["iou_weight"] * t["iou"], kw["dir_weight"] * t["dir"], kw["iou_head_weight"] * t["iou_head"]
    assert min(w_dir, w_head) > 10 * SCALAR_BAR * ref5[1] and w_iou > 10 * SCALAR_BAR * ref5[2]
    base_cls = float(m.alpha) * dev5[3] + float(m.beta) * dev5[4]
    assert dev5[1] == pytest.approx(base_cls + kw["dir_weight"] * l_dir + kw["iou_head_weight"] * l_head, rel=1e-5)
    assert dev5[0] == pytest.approx(dev5[1] + dev5[2], rel=1e-5)
    # gradients
    worst, n_zero = ("", 0.0), 0
    for k, p in got.items():
        assert p.grad is not None, k
        r = leaves[k].grad
        if O.bn_fronted_bias(k):
            assert float(p.grad.abs().max()) < ZERO_BIAS_BAR and float(r.abs().max()) < 1e-9, k
            n_zero += 1
            continue
        assert float(r.norm()) > 0, k
        l2 = float((p.grad.detach().double().cpu() - r).norm() / r.norm())
        if l2 > worst[1]:
            worst = (k, l2)
        if k in O.HEAD_KEYS or k.endswith(("deconv3.deconv.weight", "block1.0.conv.weight", "middle_layer.0.conv.weight", "vfe_1.fcn.0.weight")):
            print(f"{k:45s} relative L2 {l2:.2e}")
    print(f"composed objective, frozen masks, fp32: worst gradient relative L2 {worst[1]:.3e} ({worst[0]}); bar {O.OBJECTIVE_BAR:.1e}")
    assert n_zero == 23
    assert worst[1] < O.OBJECTIVE_BAR, worst


# -------------------------------------------------------------------------- b. the concatenation's gradient, both modes
@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_concat_gradient_across_the_two_accumulations(golden, mode, monkeypatch):
    """The same model in each mode.  A spy around dir_head.dir_head_backward clones the concatenation's gradient before and
    after each call.  Reference, per call, float64 from the device's own operands: after = before + g W (dir_ref.head_backward).
    Rows whose logit gradient is zero are bit-identical across the call (the stride gap of every row too); the others are
    within one unit in the last place of the stored type of the float64 result rounded to that type — test_gpu_dir_head's bar
    on the kernel.  The direction head's call comes first, then the IoU-aware head's, with nothing written in between, and what
    the two calls return is what the four parameters' .grad end up holding."""
    from voxelnet_amd import dir_head as DH
    from voxelnet_amd import model as M
    _, _, targets, batch = _tiny(golden)
    calls, real = [], DH.dir_head_backward

    def spy(d_logits, cat_rows, weight, d_cat):
        before = d_cat.detach().clone()
        d_w, d_b = real(d_logits, cat_rows, weight, d_cat)
        calls.append(dict(g=d_logits.detach().clone(), w=weight.detach().clone(), w_ptr=weight.data_ptr(), before=before,
                          after=d_cat.detach().clone(), d_w=d_w.detach().clone(), d_b=d_b.detach().clone()))
        return d_w, d_b
    try:
        m = _tiny_model(mode, **FULL)
        monkeypatch.setattr(DH, "dir_head_backward", spy)
        out = m(batch, DEV, targets=targets)
        out[2].backward()
        monkeypatch.setattr(DH, "dir_head_backward", real)
        torch.cuda.synchronize()
    finally:
        M.set_precision("bf16")
    mid = m.middle_rpn
    assert len(calls) == 2
    assert [c["w_ptr"] for c in calls] == [mid.dir_conv.conv.weight.data_ptr(), mid.iou_conv.conv.weight.data_ptr()]
    assert torch.equal(_bits(calls[1]["before"]), _bits(calls[0]["after"]))          # nothing else writes in between
    for c, conv, name in zip(calls, (mid.dir_conv.conv, mid.iou_conv.conv), ("direction", "IoU-aware")):
        before, after = c["before"], c["after"]
        assert before.dtype == TDT[mode] and before.dim() == 2 and before.shape[0] == 2 * 96 and before.shape[1] >= 768
        g = c["g"].permute(0, 2, 1).reshape(-1, 2).cpu().numpy().astype(np.float64)          # (B,2,S) -> (B*S, 2), row b*S + s
        listed = np.flatnonzero((g != 0).any(axis=1))
        skipped = np.ones(g.shape[0], dtype=bool)
        skipped[listed] = False
        pos_rows = np.flatnonzero((targets[0] != 0).any(axis=3).reshape(-1))
        assert listed.tolist() == pos_rows.tolist() and 0 < len(listed) < g.shape[0]          # a gradient at the positives' sites only
        sk, li = torch.from_numpy(skipped).to(DEV), torch.from_numpy(listed).to(DEV)
        assert torch.equal(_bits(after[sk]), _bits(before[sk]))
        assert torch.equal(_bits(after[:, 768:]), _bits(before[:, 768:]))
        ref_d = dir_ref.head_backward(g[listed], np.zeros((len(listed), 768)), c["w"].cpu().numpy(),
                                      before[li][:, :768].cpu().double().numpy())[0]
        want = torch.from_numpy(ref_d).to(TDT[mode])
        ulps = np.abs(_ordered(after[li][:, :768]) - _ordered(want))
        moved = int((_bits(after[li][:, :768]) != _bits(before[li][:, :768])).sum())
        print(f"{mode}, {name} head: {len(listed)} rows, d_cat max ulps {ulps.max()}, {moved} of {ulps.size} elements moved")
        assert ulps.max() <= 1
        assert moved > ulps.size // 2
        # the parameter gradients of this call are the .grad the head ends up with
        assert conv.weight.grad is not None and torch.equal(_bits(conv.weight.grad.reshape(2, 768)), _bits(c["d_w"].reshape(2, 768)))
        assert torch.equal(_bits(conv.bias.grad), _bits(c["d_b"])) and float(c["d_w"].abs().max()) > 0


# --------------------------------------------------------------------------------------- c. full-objective step equality
@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_train_step_equals_separate_calls_with_everything_on(golden, mode):
    """train_step(batch, DEV, ClipSGD) == forward + backward + step(): outputs, every .grad and every parameter bit for bit;
    the one-call step is not taken"""
    from voxelnet_amd import model as M
    from voxelnet_amd.optim import ClipSGD
    _, _, targets, batch = _tiny(golden)
    try:
        a = _tiny_model(mode, **FULL)
        oa = ClipSGD(a.parameters(), lr=1e-3, max_norm=5.0)
        assert not a._step_fused_ok(mode, oa) and not a._step_fused_ok(mode, None, targets)
        before = [p.detach().clone() for p in a.parameters()]
        out_a = a.train_step(batch, DEV, oa, targets=targets)
        b = _tiny_model(mode, **FULL)
        ob = ClipSGD(b.parameters(), lr=1e-3, max_norm=5.0)
        out_b = b(batch, DEV, targets=targets)
        out_b[2].backward()
        ob.step()
        torch.cuda.synchronize()
    finally:
        M.set_precision("bf16")
    assert len(out_a) == len(out_b) == 7
    for i, (x, y) in enumerate(zip(out_a, out_b)):
        assert torch.isfinite(x).all() and _same(x, y), (mode, i)
    pa, pb = dict(a.named_parameters()), dict(b.named_parameters())
    assert len(pa) == 108
    for k in pa:
        assert pa[k].grad is not None and torch.isfinite(pa[k].grad).all() and _same(pa[k].grad, pb[k].grad), (mode, k)
        assert _same(pa[k], pb[k]), (mode, k)
    assert any(not torch.equal(p.detach(), p0) for p, p0 in zip(a.parameters(), before))          # the step moved them
    for la, lb in ((a.last_iou, b.last_iou), (a.last_dir, b.last_dir), (a.last_iou_head, b.last_iou_head)):
        assert _same(la[0], lb[0]) and _same(la[1], lb[1]) and float(la[0]) > 0


# ------------------------------------------------------------------------------------------------ d. zero weights compose
@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_three_zero_weights_change_nothing(golden, mode):
    """iou_weight = dir_weight = iou_head_weight = 0 (every check function accepts 0): maps, the five scalars and the 104
    shared gradients are those of the focal + sine model without heads on the per-layer orchestration, bit for bit — the
    three-way version of the one-head zero-weight tests; the heads' own gradients are exactly zero"""
    from voxelnet_amd import model as M
    _, _, targets, batch = _tiny(golden)
    try:
        a = _tiny_model(mode, native=False, **FOCAL_SINE)
        assert not a._native_ok(mode)
        out_a = a(batch, DEV, targets=targets)
        out_a[2].backward()
        h = _tiny_model(mode, **dict(FULL, iou_weight=0.0, dir_weight=0.0, iou_head_weight=0.0))
        out_h = h(batch, DEV, targets=targets)
        out_h[2].backward()
        torch.cuda.synchronize()
    finally:
        M.set_precision("bf16")
    assert len(out_a) == len(out_h) == 7
    for i, (x, y) in enumerate(zip(out_a, out_h)):
        assert torch.isfinite(x).all() and _same(x, y), (mode, i)
    ga, gh = dict(a.named_parameters()), dict(h.named_parameters())
    assert len(ga) == 104 and len(gh) == 108
    for k in ga:
        assert ga[k].grad is not None and _same(ga[k].grad, gh[k].grad), (mode, k)
    for k in O.HEAD_KEYS:
        assert gh[k].grad is not None and not gh[k].grad.any(), k
    assert float(h.last_iou[0]) > 0 and float(h.last_dir[0]) > 0 and float(h.last_iou_head[0]) > 0          # computed, and weighted by 0
    assert a.last_iou is None and a.last_dir is None and a.last_iou_head is None
