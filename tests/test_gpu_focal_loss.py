"""GPU: the RPN loss with the focal classification term and / or the sine yaw term (vnLossSpec: csrc/loss.hip's k_loss with
the objective as its second template argument) against tests/focal_ref.py in float64 on the CPU, and against
itself: the separate passes, the one-pass form, the pass that also writes the heads' gradient rows, the zeroed spec against
the entry points without a spec, RPN3D.loss, the one-call train step, and a short training run.

Bars: the loss kernel's own (tests/test_gpu_loss.py) — 1e-5 relative on the five scalars, 1e-5 of the gradient's maximum
on the gradients — for every objective, the non-integer exponent (powf) included; see BARS below for the measured values.

Shapes: (3,7,5) = 105 sites, one partial workgroup, no positive in the last sample (P_b clamps to 1); (2,16,24) = 768
sites, exactly three workgroups; (2,17,15) = 510 sites, two workgroups, the second partial, the sample boundary (site 255)
inside the first."""
import ctypes
import functools
import os
from dataclasses import replace

import numpy as np
import pytest
import torch

import focal_ref
from oracle import torch_ref as tr
from test_gpu_loss import _case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ABS = (1.5, 1.0, 3.0)          # alpha, beta, sigma
SHAPES = [(3, 7, 5, True), (2, 16, 24, False), (2, 17, 15, False)]
# (cls, fa, gamma, yaw_sin): every focal combination, and the reference's cross-entropy with the sine yaw term
OBJECTIVES = [("focal", fa, gamma, ys) for gamma in (0.0, 1.0, 2.0, 2.5) for fa in (0.25, 0.5) for ys in (0, 1)] + \
             [("bce", 0.0, 0.0, 1)]
GW = (1.0, 0.3, -0.7, 0.11, 2.0)          # upstream gradients of the five outputs (tests/test_gpu_loss.py's)
# relative bars (scalars, gradients / gradient maximum): the loss kernel's own.  Measured worst over the three shapes and both
# upstream choices, MI355X: scalars 1.6e-7 for gamma in {0, 1, 2}, 1.7e-7 for gamma = 2.5 (powf), 1.1e-7 for the
# cross-entropy + sine; gradients 1.6e-7 of the maximum in all of them — the non-integer exponent meets the kernel's own bar,
# so there is no wider one for it.
BARS = (1e-5, 1e-5)


def _inputs(B, H, W, empty, seed):
    """test_gpu_loss._case — p in {0, 1, 1e-7, 1 - 1e-7} included — with the yaw targets moved so that delta_6 - tgt_6 is
    uniform in [-2, 2]: the sine is not in its linear range, and its sign changes"""
    prob, delta, pos, neg, tgt = _case(B, H, W, seed, empty)
    g = torch.Generator().manual_seed(seed + 1000)
    for a in range(2):
        tgt[..., a * 7 + 6] = delta[:, a * 7 + 6] - (torch.rand((B, H, W), generator=g) * 4 - 2)
    return prob, delta, pos, neg, tgt


def _spec(obj):
    from voxelnet_amd import model as M
    cls, fa, gamma, ys = obj
    return M.loss_spec(cls, fa, gamma, "sin" if ys else "diff")


@functools.lru_cache(maxsize=None)
def _reference(shape, obj, all_five):
    """float64 focal_ref on the CPU, once per (shape, objective, upstream): (five scalars, d_prob, d_delta)"""
    B, H, W, empty = shape
    cls, fa, gamma, ys = obj
    prob, delta, pos, neg, tgt = _inputs(B, H, W, empty, 7 + B)
    p64, d64 = prob.double().requires_grad_(True), delta.double().requires_grad_(True)
    out = torch.stack(focal_ref.loss(p64, d64, pos.double(), neg.double(), tgt.double(), *ABS, cls=cls, fa=fa, gamma=gamma,
                                     yaw="sin" if ys else "diff"))
    ((out * torch.tensor(GW, dtype=torch.float64)).sum() if all_five else out[0]).backward()
    return out.detach().numpy(), p64.grad, d64.grad


def _dev(B, H, W, empty, seed):
    return tuple(t.to(DEV).contiguous() for t in _inputs(B, H, W, empty, seed))


def _ptrs(ts):
    return [t.data_ptr() for t in ts]


@pytest.mark.parametrize("obj", OBJECTIVES, ids=lambda o: f"{o[0]}-fa{o[1]}-g{o[2]}-sin{o[3]}")
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(v) for v in s[:3]))
def test_scalars_and_gradients_against_focal_ref(shape, obj):
    """check 1: the five scalars and both gradients, with all five upstream gradients set and with only the loss's"""
    from voxelnet_amd import model as M
    B, H, W, empty = shape
    prob, delta, pos, neg, tgt = _dev(B, H, W, empty, 7 + B)
    spec = _spec(obj)
    for all_five in (True, False):
        ref, rp, rd = _reference(shape, obj, all_five)
        pg, dg = prob.clone().requires_grad_(True), delta.clone().requires_grad_(True)
        out = M._LossFn.apply(pg, dg, pos, neg, tgt, *ABS, spec)
        (sum(o * w for o, w in zip(out, GW)) if all_five else out[0]).backward()
        got = np.array([o.item() for o in out], dtype=np.float64)
        es = float(np.max(np.abs(got - ref) / np.abs(ref)))
        eg = max((g.cpu().double() - r).abs().max().item() / r.abs().max().item() for g, r in ((pg.grad, rp), (dg.grad, rd)))
        print(f"{shape[:3]} {obj} all_five={all_five}: scalars {es:.2e}, gradients {eg:.2e} of the maximum")
        assert np.isfinite(got).all() and torch.isfinite(pg.grad).all() and torch.isfinite(dg.grad).all()
        assert np.isfinite(ref).all() and rp.abs().max().item() > 0 and rd.abs().max().item() > 0
        assert es <= BARS[0], (got, ref)
        assert eg <= BARS[1]


@pytest.mark.parametrize("obj", OBJECTIVES, ids=lambda o: f"{o[0]}-fa{o[1]}-g{o[2]}-sin{o[3]}")
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(v) for v in s[:3]))
def test_one_pass_equals_the_two_passes_bit_for_bit(shape, obj):
    """check 2: vn_rpn_loss_norm + vn_rpn_loss_spec_fwd_bwd + vn_rpn_loss_finalize against vn_rpn_loss_spec_fwd +
    vn_rpn_loss_spec_bwd: scalars and gradients bit-identical, all five upstream gradients and the loss's alone"""
    from voxelnet_amd import _lib
    B, H, W, empty = shape
    ins = _dev(B, H, W, empty, 21 + B)
    prob, delta = ins[0], ins[1]
    sp = ctypes.byref(_spec(obj))
    wsb = _lib.load().vn_rpn_loss_workspace_bytes(B, H, W)
    st = _lib.raw_stream()
    gw = [torch.tensor([v], device=DEV) for v in GW]
    for ups in (gw, [gw[0], None, None, None, None]):
        gp = [None if g is None else g.data_ptr() for g in ups]
        ws_a = torch.zeros(wsb, dtype=torch.uint8, device=DEV)
        out_a = torch.empty(5, device=DEV)
        dp_a, dd_a = torch.empty_like(prob), torch.empty_like(delta)
        _lib.call("vn_rpn_loss_spec_fwd", *_ptrs(ins), B, H, W, *ABS, ws_a.data_ptr(), wsb, out_a.data_ptr(), st, sp)
        _lib.call("vn_rpn_loss_spec_bwd", *_ptrs(ins), B, H, W, *ABS, ws_a.data_ptr(), *gp, dp_a.data_ptr(), dd_a.data_ptr(), st, sp)
        ws_b = torch.full((wsb,), 255, dtype=torch.uint8, device=DEV)
        out_b = torch.empty(5, device=DEV)
        dp_b, dd_b = torch.empty_like(prob), torch.empty_like(delta)
        _lib.call("vn_rpn_loss_norm", ins[2].data_ptr(), ins[3].data_ptr(), B, H, W, ws_b.data_ptr(), wsb, st)
        _lib.call("vn_rpn_loss_spec_fwd_bwd", *_ptrs(ins), B, H, W, *ABS, ws_b.data_ptr(), wsb, *gp, dp_b.data_ptr(),
                  dd_b.data_ptr(), st, sp)
        _lib.call("vn_rpn_loss_finalize", ws_b.data_ptr(), wsb, B, H, W, ABS[0], ABS[1], out_b.data_ptr(), st)
        torch.cuda.synchronize()
        assert torch.equal(out_a, out_b), (out_a, out_b)
        assert torch.equal(dp_a, dp_b) and torch.equal(dd_a, dd_b)
        assert torch.isfinite(out_a).all() and torch.isfinite(dp_a).all() and torch.isfinite(dd_a).all()


ROW_OBJECTIVES = [("focal", 0.25, 2.0, 1), ("focal", 0.5, 2.5, 0), ("focal", 0.25, 0.0, 1), ("bce", 0.0, 0.0, 1)]
TAIL = 5                         # sentinel rows behind the (B*S, stride) buffer


@pytest.mark.parametrize("form", ["f32", "bf16", "split"])
@pytest.mark.parametrize("obj", ROW_OBJECTIVES, ids=lambda o: f"{o[0]}-fa{o[1]}-g{o[2]}-sin{o[3]}")
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(v) for v in s[:3]))
def test_rows_pass_equals_heads_bwd_on_its_own_gradients(shape, obj, form):
    """check 3: vn_rpn_loss_spec_fwd_bwd_rows — what vn_net_step launches — writes the gradients and partial sums of
    vn_rpn_loss_spec_fwd_bwd, and the (B*S, 16) rows vn_heads_bwd makes of its own d_prob / d_delta, bit for bit, as fp32
    rows, bf16 rows and split rows (hi | lo, stride 32); the sentinel rows behind B*S are not touched"""
    from voxelnet_amd import _lib
    B, H, W, empty = shape
    ins = _dev(B, H, W, empty, 33 + B)
    prob, delta = ins[0], ins[1]
    sp = ctypes.byref(_spec(obj))
    wsb = _lib.load().vn_rpn_loss_workspace_bytes(B, H, W)
    st = _lib.raw_stream()
    g = torch.tensor([0.7], device=DEV)
    S = H * W
    rdt, cdt, stride, split, idt, fill = {"f32": (torch.float32, _lib.VN_F32, 16, 0, torch.int32, 0x4B4B4B4B),
                                          "bf16": (torch.bfloat16, _lib.VN_BF16, 16, 0, torch.int16, 0x4B4B),
                                          "split": (torch.bfloat16, _lib.VN_BF16, 32, 1, torch.int16, 0x4B4B)}[form]

    def rows():
        return torch.full((B * S + TAIL, stride), fill, dtype=idt, device=DEV)
    # the pass without rows, then vn_heads_bwd on what it wrote
    ws_a = torch.zeros(wsb, dtype=torch.uint8, device=DEV)
    dp_a, dd_a, rows_a = torch.empty_like(prob), torch.empty_like(delta), rows()
    _lib.call("vn_rpn_loss_norm", ins[2].data_ptr(), ins[3].data_ptr(), B, H, W, ws_a.data_ptr(), wsb, st)
    _lib.call("vn_rpn_loss_spec_fwd_bwd", *_ptrs(ins), B, H, W, *ABS, ws_a.data_ptr(), wsb, g.data_ptr(), None, None, None, None,
              dp_a.data_ptr(), dd_a.data_ptr(), st, sp)
    _lib.call("vn_heads_bwd", dp_a.data_ptr(), dd_a.data_ptr(), prob.data_ptr(), B, S, rows_a.data_ptr(), cdt, stride, split, st)
    # the rows pass
    ws_b = torch.zeros(wsb, dtype=torch.uint8, device=DEV)
    dp_b, dd_b, rows_b = torch.empty_like(prob), torch.empty_like(delta), rows()
    _lib.call("vn_rpn_loss_norm", ins[2].data_ptr(), ins[3].data_ptr(), B, H, W, ws_b.data_ptr(), wsb, st)
    _lib.call("vn_rpn_loss_spec_fwd_bwd_rows", *_ptrs(ins), B, H, W, *ABS, ws_b.data_ptr(), wsb, g.data_ptr(), dp_b.data_ptr(),
              dd_b.data_ptr(), rows_b.data_ptr(), cdt, stride, split, st, sp)
    torch.cuda.synchronize()
    assert torch.equal(dp_a, dp_b) and torch.equal(dd_a, dd_b) and torch.equal(ws_a, ws_b)
    assert torch.isfinite(dp_b).all() and torch.isfinite(dd_b).all()
    assert torch.equal(rows_a, rows_b)
    assert bool((rows_b[B * S:] == fill).all()), "rows behind B*S were written"
    assert bool((rows_b[:B * S] != fill).any(dim=0).all()), "a column of the rows was never written"
    assert torch.isfinite(rows_b[:B * S].view(rdt).float()).all()
    # and the rows are what the definition says: d_prob * p * (1 - p) on the stored values, then the 14 regression gradients
    if form == "f32":
        want = torch.cat([dp_b * prob * (1.0 - prob), dd_b], dim=1).permute(0, 2, 3, 1).reshape(B * S, 16)
        assert torch.equal(rows_b[:B * S].view(torch.float32), want)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(v) for v in s[:3]))
def test_zeroed_spec_is_the_old_entry_points_bit_for_bit(shape):
    """check 4: fwd, bwd, the one-pass form and the rows pass with a zeroed vnLossSpec, and with NULL, against the entry
    points without a spec"""
    from voxelnet_amd import _lib
    B, H, W, empty = shape
    ins = _dev(B, H, W, empty, 45 + B)
    prob, delta = ins[0], ins[1]
    wsb = _lib.load().vn_rpn_loss_workspace_bytes(B, H, W)
    st = _lib.raw_stream()
    gw = [torch.tensor([v], device=DEV) for v in GW]
    gp = [g.data_ptr() for g in gw]
    S = H * W

    def run(spec_args, sfx):
        res = []
        ws = torch.zeros(wsb, dtype=torch.uint8, device=DEV)
        out = torch.empty(5, device=DEV)
        dp, dd = torch.empty_like(prob), torch.empty_like(delta)
        _lib.call(f"vn_rpn_loss{sfx}_fwd", *_ptrs(ins), B, H, W, *ABS, ws.data_ptr(), wsb, out.data_ptr(), st, *spec_args)
        _lib.call(f"vn_rpn_loss{sfx}_bwd", *_ptrs(ins), B, H, W, *ABS, ws.data_ptr(), *gp, dp.data_ptr(), dd.data_ptr(), st, *spec_args)
        res += [out, dp, dd, ws]
        ws2 = torch.zeros(wsb, dtype=torch.uint8, device=DEV)
        out2 = torch.empty(5, device=DEV)
        dp2, dd2 = torch.empty_like(prob), torch.empty_like(delta)
        _lib.call("vn_rpn_loss_norm", ins[2].data_ptr(), ins[3].data_ptr(), B, H, W, ws2.data_ptr(), wsb, st)
        _lib.call(f"vn_rpn_loss{sfx}_fwd_bwd", *_ptrs(ins), B, H, W, *ABS, ws2.data_ptr(), wsb, *gp, dp2.data_ptr(), dd2.data_ptr(), st,
                  *spec_args)
        _lib.call("vn_rpn_loss_finalize", ws2.data_ptr(), wsb, B, H, W, ABS[0], ABS[1], out2.data_ptr(), st)
        res += [out2, dp2, dd2, ws2]
        ws3 = torch.zeros(wsb, dtype=torch.uint8, device=DEV)
        dp3, dd3 = torch.empty_like(prob), torch.empty_like(delta)
        rows = torch.zeros((B * S, 16), dtype=torch.int16, device=DEV)
        _lib.call("vn_rpn_loss_norm", ins[2].data_ptr(), ins[3].data_ptr(), B, H, W, ws3.data_ptr(), wsb, st)
        _lib.call(f"vn_rpn_loss{sfx}_fwd_bwd_rows", *_ptrs(ins), B, H, W, *ABS, ws3.data_ptr(), wsb, gp[0], dp3.data_ptr(),
                  dd3.data_ptr(), rows.data_ptr(), _lib.VN_BF16, 16, 0, st, *spec_args)
        torch.cuda.synchronize()
        return res + [dp3, dd3, rows, ws3]
    old = run((), "")
    assert torch.isfinite(old[0]).all()
    for spec_args in ((ctypes.byref(_lib.VnLossSpec()),), (None,)):
        new = run(spec_args, "_spec")
        assert len(new) == len(old) and all(torch.equal(a, b) for a, b in zip(old, new))


def test_module_loss_equals_focal_ref():
    """check 5: RPN3D("Car", cls_loss="focal", yaw_loss="sin").loss on numpy targets, values and gradients; the default model
    beside it still computes the reference's loss"""
    from voxelnet_amd import model as M
    shape = (2, 17, 15, False)
    obj = ("focal", 0.25, 2.0, 1)
    B, H, W, empty = shape
    prob, delta, pos, neg, tgt = _inputs(B, H, W, empty, 7 + B)
    m = M.RPN3D("Car", cls_loss="focal", yaw_loss="sin").to(DEV)
    assert (m.focal_alpha, m.focal_gamma) == (0.25, 2.0) and ABS == (m.alpha, m.beta, m.sigma)
    pg, dg = prob.to(DEV).requires_grad_(True), delta.to(DEV).requires_grad_(True)
    out = m.loss(pg, dg, pos.numpy(), neg.numpy(), tgt.numpy())
    assert len(out) == 5 and all(o.dim() == 0 for o in out)
    out[0].backward()
    ref, rp, rd = _reference(shape, obj, False)
    np.testing.assert_allclose([o.item() for o in out], ref, rtol=1e-5, atol=0)
    for got, want in ((pg.grad, rp), (dg.grad, rd)):
        assert (got.cpu().double() - want).abs().max().item() <= 1e-5 * want.abs().max().item()
    d = M.RPN3D("Car").to(DEV).loss(prob.to(DEV), delta.to(DEV), pos.numpy(), neg.numpy(), tgt.numpy())
    want = tr.rpn_loss(prob.double(), delta.double(), pos.double(), neg.double(), tgt.double(), *ABS)
    np.testing.assert_allclose([o.item() for o in d], [w.item() for w in want], rtol=1e-5)
    assert abs(d[1].item() - out[1].item()) > 0.1 * abs(d[1].item())       # (the two objectives are not the same number)


# ---- the train step on the tiny golden batch (tests/golden/middle_tiny_car.npz + rpn3d_tiny.npz: 10 x 16 x 24 grid, B = 2,
# 8 x 12 maps, 17 + 16 positive anchors) with focal + sine
FOCAL = dict(cls_loss="focal", focal_alpha=0.25, focal_gamma=2.0, yaw_loss="sin")


def _tiny(golden):
    g, t = golden("middle_tiny_car"), golden("rpn3d_tiny")
    lens = [int(x) for x in g["feat_lens"]]
    feats = list(torch.split(torch.from_numpy(g["features"]), lens))
    coords = list(torch.split(torch.from_numpy(g["coords"]), lens))
    targets = tuple(np.ascontiguousarray(t[k], dtype=np.float32) for k in ("pos", "neg", "targets"))
    return feats, coords, targets


def _tiny_model(mode, **kw):
    from voxelnet_amd import model as M
    M.set_precision(mode)
    m = M.RPN3D("Car", **kw)
    m.load_state_dict(tr.make_state_dict("Car"))
    m.feature_net._grid = replace(m.feature_net._grid, H=16, W=24)
    return m.to(DEV).train()


@functools.lru_cache(maxsize=None)
def _tiny_oracle():
    """focal_ref on the maps of the CPU oracle's float64 train-mode forward of the tiny batch, differentiated back to
    every parameter: ({parameter: gradient}, the five scalars)"""
    g, t = (np.load(os.path.join(GOLDEN, n + ".npz")) for n in ("middle_tiny_car", "rpn3d_tiny"))
    lens = [int(x) for x in g["feat_lens"]]
    feats = [f.double() for f in torch.split(torch.from_numpy(g["features"]), lens)]
    coords = list(torch.split(torch.from_numpy(g["coords"]), lens))
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in tr.make_state_dict("Car").items()}
    keys = tr.param_keys(sd)
    leaves = {k: sd[k].detach().clone().requires_grad_(True) for k in keys}
    work = dict(sd)
    work.update(leaves)
    prob, reg = tr.middle_rpn(tr.feature_net(feats, coords, work, (10, 16, 24), True), work, "Car", True)
    pos, neg, tgt = (torch.from_numpy(np.asarray(t[k], dtype=np.float32)).double() for k in ("pos", "neg", "targets"))
    out = focal_ref.loss(prob, reg, pos, neg, tgt, *ABS, cls="focal", fa=0.25, gamma=2.0, yaw="sin")
    out[0].backward()
    return {k: leaves[k].grad for k in keys}, [float(o) for o in out]


# first and last layer of the network: the encoder's first linear map (its bias feeds a BatchNorm: gradient 0) and the heads
ENDS = ("feature_net.vfe_1.fcn.0.weight", "middle_rpn.prob_conv.conv.weight", "middle_rpn.prob_conv.conv.bias",
        "middle_rpn.reg_conv.conv.weight", "middle_rpn.reg_conv.conv.bias")


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_train_step_with_focal_and_sine(golden, mode):
    """check 6: RPN3D.train_step as ONE call (vn_net_step with the spec in its tail) equals forward + backward as separate
    module calls bit for bit — maps, the five loss scalars, every .grad — and is not the default objective's step; in fp32
    the gradients of the first and the last layer match focal_ref driven through the CPU oracle's float64 forward at
    relative L2 <= 0.1, the bar tests/test_gpu_model.py::test_car_full_backward sets for fp32 gradients chained through the
    23 layers against that oracle (measured here: 2.5e-5 on the encoder's first weight, <= 1.3e-5 on the heads)"""
    from voxelnet_amd import model as M
    feats, coords, targets = _tiny(golden)
    batch = (None, None, [f.to(DEV) for f in feats], None, [c.to(DEV) for c in coords], None, None)
    try:
        a = _tiny_model(mode, **FOCAL)
        assert a._step_fused_ok(mode, None)
        out_a = a.train_step(batch, DEV, None, targets=targets)
        b = _tiny_model(mode, **FOCAL)
        out_b = b(batch, DEV, targets=targets)
        out_b[2].backward()
        c = _tiny_model(mode)
        out_c = c.train_step(batch, DEV, None, targets=targets)
        torch.cuda.synchronize()
    finally:
        M.set_precision("bf16")
    assert len(out_a) == len(out_b) == 7
    for i, (x, y) in enumerate(zip(out_a, out_b)):
        assert torch.isfinite(x).all() and torch.equal(x, y), (mode, "output", i)
    ga, gb = dict(a.named_parameters()), dict(b.named_parameters())
    for k in ga:
        assert ga[k].grad is not None and torch.isfinite(ga[k].grad).all(), k
        assert torch.equal(ga[k].grad, gb[k].grad), (mode, k)
    assert torch.equal(out_a[0], out_c[0]) and float(out_a[2]) != float(out_c[2])        # same maps, another loss
    if mode == "fp32":
        ref, scalars = _tiny_oracle()
        np.testing.assert_allclose([float(o) for o in out_a[2:]], scalars, rtol=2e-3)     # (test_rpn3d_forward_loss's bar)
        for k in ENDS:
            r = ref[k].numpy()
            l2 = float(np.linalg.norm(ga[k].grad.cpu().numpy().astype(np.float64) - r) / np.linalg.norm(r))
            print(f"{k}: relative L2 {l2:.2e}")
            assert np.linalg.norm(r) > 0 and l2 <= 0.1, (k, l2)


def test_ten_adamw_steps_in_focal_mode_lower_the_loss(golden):
    """check 7: ten ClipAdamW steps on the tiny batch, focal + sine, bf16 (the one-call step, the optimizer after it): the
    loss ends lower than it starts (measured: 21.21 -> 2.44), every parameter stays finite"""
    from voxelnet_amd import model as M
    from voxelnet_amd.optim import ClipAdamW
    feats, coords, targets = _tiny(golden)
    batch = (None, None, [f.to(DEV) for f in feats], None, [c.to(DEV) for c in coords], None, None)
    try:
        m = _tiny_model("bf16", **FOCAL)
        opt = ClipAdamW(list(m.parameters()), lr=1e-3, max_norm=5.0)
        losses = []
        for _ in range(10):
            assert m._step_fused_ok("bf16", opt)
            out = m.train_step(batch, DEV, opt, targets=targets)
            losses.append(out[2])
            opt.zero_grad(set_to_none=True)
        losses = [float(x) for x in losses]
    finally:
        M.set_precision("bf16")
    print("focal + sine, ten ClipAdamW steps:", " ".join(f"{x:.4f}" for x in losses))
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    assert all(torch.isfinite(p).all() for p in m.parameters())
