"""GPU: eval-mode inference (model.eval(), then RPN3D.detect — the reference's validation loop, the maps RPN3D.predict reads)
at FULL size against a float64 oracle.

Why a test of its own.  Every other full-size test runs the network in train mode, and train-mode BatchNorm removes any
per-channel offset (and any positive per-channel scale) that reaches it: a conv bias dropped, doubled or taken from the
wrong layer, or one output channel of a packed weight scaled, moves the train-mode maps by 1e-12 .. 1e-7 and the eval-mode
maps by 1e-3 .. 1 (test_car_oracle_eval_maps_see_biases_and_statistics holds that power in place).  In eval mode the
native executor (csrc/runtime.hip) also takes routes that training never takes: the conv epilogues without statistics
(slab = nullptr), the BatchNorm from the running statistics (vn_bn_finalize, training = 0), the first layer without its
bias fill (the flagged apply computes every unreached site from the bias) and the VFE with training = 0.

Running statistics.  Defaults (0 / 1) or one momentum-0.1 step would leave them near the identity, so each config gets
FOREIGN statistics: one float64 train-mode oracle forward on a different batch of the same workload with
oracle.torch_ref.BN_MOMENTUM = 1.0 fills all 25 BatchNorms (the VFE's included) with that batch's mean and unbiased
variance.  The model and the oracle then hold the same (fp32-valued) statistics.

Bars (measured values beside them): maps as max error / map maximum, per config and mode; layers as relative L2 and max
error / maximum against a float64 single-layer oracle fed the executor's own input read from its arena (bf16: half a
bf16 ulp, test_gpu_bf16_parity.assert_rounded)."""
import ctypes
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import torch_ref as tr
from test_gpu_bf16_parity import assert_rounded, emulate_fp32_bn, oracle_conv64, rows_to_nchw64
from test_gpu_native_chain import (DEV, MODES, arena_tensor, car_inputs, dead_bias, dense_inputs,  # noqa: F401 (fixtures)
                                   ped_inputs, rel_err, state_dict_f64, tensor_info)

pytestmark = pytest.mark.gpu

# config -> (class, workload id of synth.workload_frames): the inputs are test_gpu_native_chain's fixtures
CONFIGS = {"car": ("Car", 2), "ped": ("Pedestrian", 3), "dense": ("Car", 5)}
# eval maps, max error / map maximum (prob and reg), whole batch and per sample: about 3x the measured worst, below the
# ceilings 1e-4 (fp32) and 1e-3 (fp32x3).  bf16: a report bar, measured + margin (part c: the layers are held below)
MAP_BARS = {
    ("car", "fp32"): 4e-5,       # 1.25e-5 / 6.7e-6 (eval with grad enabled, part f: 1.9e-5 / 7.7e-6)
    ("car", "fp32x3"): 4e-4,     # 1.30e-4 / 8.4e-5
    ("ped", "fp32"): 4e-5,       # 1.33e-5 / 8.0e-6
    ("ped", "fp32x3"): 6e-4,     # 1.83e-4 / 1.02e-4
    ("dense", "fp32"): 5e-5,     # 1.64e-5 / 9.3e-6
    ("dense", "fp32x3"): 4e-4,   # 1.23e-4 / 8.9e-5
    ("car", "bf16"): 0.15,       # 8.6e-2 / 4.5e-2
    ("ped", "bf16"): 0.15,       # 8.6e-2 / 5.7e-2
    ("dense", "bf16"): 0.15,     # 7.4e-2 / 6.0e-2
}
# every layer's y and a against the float64 single-layer oracle on the executor's own input: (relative L2, max error /
# maximum), about 3x the worst layer measured (car and dense)
LAYER_BARS = {"fp32": (2e-6, 5e-6),       # 6.6e-7 (block3.4 a) / 1.6e-6 (middle_layer.2 a, dense)
              "fp32x3": (1.5e-5, 3e-5)}   # 5.1e-6 / 9.2e-6 (block3.5 a)
# the heads from the concatenation (prob and reg, max error / maximum)
HEAD_BARS = {"fp32": 2.5e-6,    # 8.3e-7
             "fp32x3": 3e-5,    # 9.2e-6
             "bf16": 1e-6}      # 3.5e-7 (bf16 layers: the assert_rounded bar; measured worst rel-L2 1.7e-3)


def _frames(config_id, batch, grid, frame0):
    from voxelnet_amd import synth
    from voxelnet_amd.voxelize import voxelize_device
    feats, coords = [], []
    for b, f in enumerate(synth.workload_frames(config_id, batch=batch, frame0=frame0)):
        fb, cb, _ = voxelize_device(torch.from_numpy(f).to(DEV), grid, b, coord_cols=4)
        feats.append(fb)
        coords.append(cb)
    return feats, coords


def _is_running(k):
    return k.endswith("running_mean") or k.endswith("running_var")


def _eval_context(tag, inp):
    """foreign running statistics for config `tag` and the float64 oracle's eval maps of `inp` under them (computed once
    per config, shared by every mode)"""
    cls, config_id = CONFIGS[tag]
    grid, B = inp["grid"], len(inp["feats"])
    t0 = time.perf_counter()
    sd = state_dict_f64(cls)
    ff, fc = _frames(config_id, B, grid, frame0=B)             # the next B frames of the workload: another batch
    with pytest.MonkeyPatch.context() as mp, torch.no_grad():
        mp.setattr(tr, "BN_MOMENTUM", 1.0)                       # running statistics := that batch's mean / unbiased var
        tr.middle_rpn(tr.feature_net([f.cpu().double() for f in ff], [c.cpu() for c in fc], sd, grid.dims, True), sd, cls, True)
    for k in sd:
        if _is_running(k):
            sd[k] = sd[k].float().double()                       # what the fp32 model holds: the oracle uses the same values
    assert sum(k.endswith("running_var") for k in sd) == 25
    sd32 = {k: (v.float() if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    t1 = time.perf_counter()
    with torch.no_grad():
        rp, rr = tr.middle_rpn(tr.feature_net(inp["feats64"], inp["coords_cpu"], sd, grid.dims, False), sd, cls, False)
    print(f"\n{tag}: foreign statistics (float64 train forward, momentum 1) {t1 - t0:.1f} s, float64 eval maps "
          f"{time.perf_counter() - t1:.1f} s; VFE running var mean {float(sd['feature_net.vfe_1.bn.running_var'].mean()):.1f}"
          f" / {float(sd['feature_net.vfe_2.bn.running_var'].mean()):.1f}")
    return dict(cls=cls, sd=sd, sd32=sd32, rp=rp, rr=rr)


@pytest.fixture(scope="module")
def car_eval(car_inputs):  # noqa: F811
    return _eval_context("car", car_inputs)


@pytest.fixture(scope="module")
def ped_eval(ped_inputs):  # noqa: F811
    return _eval_context("ped", ped_inputs)


@pytest.fixture(scope="module")
def dense_eval(dense_inputs):  # noqa: F811
    return _eval_context("dense", dense_inputs)


def _model(cls, sd32, mode, grid):
    from voxelnet_amd import model as M
    M.set_precision(mode)
    m = M.RPN3D(cls)
    m.load_state_dict(sd32)
    m.feature_net._grid = grid
    return m.to(DEV)


def native_eval(cls, inp, mode, sd32, keep=None):
    """model.eval(); detect under no_grad on the native executor.  keep(ws, cfg, K, m): called after the forward (the
    arena holds it).  -> (prob, reg)"""
    from voxelnet_amd import _lib
    from voxelnet_amd import model as M
    m = _model(cls, sd32, mode, inp["grid"]).eval()
    assert m._native_ok(mode) and m.sparse_first_layer and not m.training
    seen, cfgs = [], []
    acquire, call = M.RPN3D._ws_acquire, _lib.call

    def spy(self, nbytes, device):
        ws = acquire(self, nbytes, device)
        seen.append((ws, nbytes))
        return ws

    def call_spy(name, *args):
        if name == "vn_net_forward":
            cfgs.append(_lib.VnNetConfig.from_buffer_copy(args[1]._obj))      # the configuration of the call, as passed
        return call(name, *args)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(M.RPN3D, "_ws_acquire", spy)
        mp.setattr(_lib, "call", call_spy)
        with torch.no_grad():
            prob, reg = m.detect(inp["feats"], inp["coords"])
    torch.cuda.synchronize()
    assert len(seen) == 1 and len(cfgs) == 1, "the eval forward did not run on the native executor"
    assert cfgs[0].training == 0 and cfgs[0].sparse_first == 1 and cfgs[0].mode == MODES[mode], "not the eval-mode executor"
    ws, nbytes = seen[0]
    D, H, W = inp["grid"].dims
    B, K = len(inp["feats"]), sum(int(f.shape[0]) for f in inp["feats"])
    cfg = _lib.VnNetConfig(B, D, H, W, m.middle_rpn._block1_stride, MODES[mode], 0, 1, 0, 0, 0, 0)
    assert all(getattr(cfg, f) == getattr(cfgs[0], f) for f in ("B", "D", "H", "W", "block1_stride", "grad_storage"))
    assert _lib.load().vn_net_workspace_bytes(ctypes.byref(cfg), K) == nbytes      # the plan the query walks is this one
    if keep is not None:
        keep(ws, cfg, K, m)
    return prob.detach(), reg.detach()


def _map_errors(prob, reg, rp, rr):
    """max error / maximum of prob and reg: the whole batch, then each sample"""
    out = [(rel_err(prob, rp), rel_err(reg, rr))]
    for b in range(prob.shape[0]):
        out.append((rel_err(prob[b], rp[b]), rel_err(reg[b], rr[b])))
    return out


# ---- (b) the oracle keeps the power to see eval-only errors ---------------------------------------------------------

def test_car_oracle_eval_maps_see_biases_and_statistics(car_eval, car_inputs):  # noqa: F811
    """at oracle level, car B = 2: the eval maps under the foreign statistics differ from the train-mode maps of the same
    batch, and from the eval maps with the 23 conv / deconv biases in front of a BatchNorm set to 0, by more than 100x the
    fp32 map bar — nobody can make the tests below pass by going back to default statistics or to train mode"""
    sd, cls, dims = car_eval["sd"], car_eval["cls"], car_inputs["grid"].dims
    bar = 100 * MAP_BARS[("car", "fp32")]
    f64, c = car_inputs["feats64"], car_inputs["coords_cpu"]
    with torch.no_grad():
        work = {k: (v.clone() if _is_running(k) else v) for k, v in sd.items()}      # (train mode updates them in place)
        tp, trg = tr.middle_rpn(tr.feature_net(f64, c, work, dims, True), work, cls, True)
        zero = {k: (torch.zeros_like(v) if dead_bias(k) else v) for k, v in sd.items()}
        assert sum(map(dead_bias, sd)) == 23
        zp, zr = tr.middle_rpn(tr.feature_net(f64, c, zero, dims, False), zero, cls, False)
    rp, rr = car_eval["rp"], car_eval["rr"]
    et, ez = (rel_err(tp, rp), rel_err(trg, rr)), (rel_err(zp, rp), rel_err(zr, rr))
    print(f"car oracle: eval vs train maps {et[0]:.3g} / {et[1]:.3g}, eval with the biases zeroed {ez[0]:.3g} / {ez[1]:.3g} "
          f"(must exceed {bar:.0e})")
    assert min(et) > bar and min(ez) > bar, (et, ez)


# ---- (c) the whole network on the native executor -------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["fp32", "fp32x3", "bf16"])
@pytest.mark.parametrize("config", ["car", "ped", "dense"])
def test_native_eval_maps_vs_float64(config, mode, request):
    """car B = 2, ped B = 2, dense B = 1 (test_gpu_native_chain's inputs) under foreign running statistics: model.eval(),
    detect under no_grad on the native executor with cfg.training == 0, maps against the float64 oracle's eval maps"""
    from voxelnet_amd import model as M
    ctx, inp = request.getfixturevalue(f"{config}_eval"), request.getfixturevalue(f"{config}_inputs")
    t0 = time.perf_counter()
    try:
        prob, reg = native_eval(ctx["cls"], inp, mode, ctx["sd32"])
    finally:
        M.set_precision("bf16")
    errs = _map_errors(prob, reg, ctx["rp"], ctx["rr"])
    bar = MAP_BARS[(config, mode)]
    print(f"{config} {mode} eval maps vs float64: batch prob {errs[0][0]:.2e} reg {errs[0][1]:.2e}; per sample "
          + ", ".join(f"{p:.2e} / {r:.2e}" for p, r in errs[1:]) + f" (bar {bar:.0e}); {time.perf_counter() - t0:.1f} s")
    assert torch.isfinite(prob).all() and torch.isfinite(reg).all()
    assert max(max(e) for e in errs) < bar, errs


# ---- (d) layer by layer, from the arena -----------------------------------------------------------------------------

def _to_oracle(t, name, spec):
    """a (B,D,H,W,C) rows tensor of layer `name` -> the oracle's NC(D)HW float64 (host); middle_layer.2's BEV activation
    (B,1,H,W,128), channel d*64 + c -> (B,64,2,H,W)"""
    if name == "middle_layer.2" and t.shape[1] == 1:
        B, H, W = t.shape[0], t.shape[2], t.shape[3]
        return t.reshape(B, H, W, 2, 64).permute(0, 4, 3, 1, 2).double().cpu().contiguous()
    return rows_to_nchw64(t, spec.dim)


def _active_sites(coord, B, dims):
    """middle_layer.0's output sites an occupied voxel reaches (the 3x3x3 window, stride (2,1,1), padding 1), (B,D',H,W)"""
    D, H, W = dims
    c = coord.long().cpu()
    occ = torch.zeros((B, 1, D, H, W), dtype=torch.float32)
    occ[c[:, 0], 0, c[:, 1], c[:, 2], c[:, 3]] = 1.0
    return F.conv3d(occ, torch.ones((1, 1, 3, 3, 3)), stride=(2, 1, 1), padding=1)[:, 0] > 0


def _dist(got, ref):
    d = got - ref
    return float(d.norm() / (ref.norm() + 1e-30)), float(d.abs().max() / ref.abs().max().clamp(min=1e-30))


@pytest.mark.parametrize("config,mode", [("car", "fp32"), ("car", "fp32x3"), ("car", "bf16"), ("dense", "fp32")])
def test_native_eval_layers_vs_float64_on_own_input(config, mode, request):
    """after the eval forward, every layer's y, a and statistics from the arena (vn_net_tensor_info on the eval
    configuration): the statistics are the running-derived ones, and each layer's y = conv + bias and a = relu(BN_running(y))
    match a float64 single-layer oracle fed the executor's own input — a wrong bias, a stale statistic or a mis-wired
    layer fails at the layer where it happens.  middle_layer.0's y only at its active sites (eval leaves the others
    unwritten by design), its a everywhere; the heads from the concatenation last."""
    from voxelnet_amd import _lib
    from voxelnet_amd import model as M
    from voxelnet_amd import net as N
    ctx, inp = request.getfixturevalue(f"{config}_eval"), request.getfixturevalue(f"{config}_inputs")
    sd32, cls = ctx["sd32"], ctx["cls"]
    saved = {}

    def keep(ws, cfg, K, m):
        table = N.layer_table(m.middle_rpn._block1_stride)
        for l, (name, spec) in enumerate(table):
            st = arena_tensor(ws, tensor_info(cfg, K, l, _lib.VN_NET_STATS)).reshape(4, spec.cout).double().cpu()
            saved[name] = (arena_tensor(ws, tensor_info(cfg, K, l, _lib.VN_NET_Y)),
                           arena_tensor(ws, tensor_info(cfg, K, l, _lib.VN_NET_A)), st)
        saved["cat"] = arena_tensor(ws, tensor_info(cfg, K, len(table) - 1, _lib.VN_NET_A), C=768)
        saved["table"] = table
        # middle_layer.0's input: the voxel features as the executor read them (the eval VFE is per voxel: deterministic)
        fn = m.feature_net
        vw, _, _ = M.featnet_forward(torch.cat(inp["feats"], 0).contiguous(), [p.detach() for p in M._vfe_weights(fn)],
                                     fn._bufs(), False)
        saved["vw"] = (vw.bfloat16().float() if mode == "bf16" else vw).double().cpu()
    t0 = time.perf_counter()
    try:
        prob, reg = native_eval(cls, inp, mode, sd32, keep=keep)
    finally:
        M.set_precision("bf16")
    t1 = time.perf_counter()
    rows, eh = check_layers(saved, sd32, mode, torch.cat(inp["coords_cpu"], 0), len(inp["feats"]), inp["grid"].dims, prob, reg,
                            config)
    for name, ey, ea in rows:
        print(f"   {config} {mode} {name:16s} y rel-L2 {ey[0]:.2e} max {ey[1]:.2e} | a rel-L2 {ea[0]:.2e} max {ea[1]:.2e}")
    wy = max(rows, key=lambda r: max(r[1]))
    wa = max(rows, key=lambda r: max(r[2]))
    print(f"{config} {mode} eval layers vs float64 on the executor's own input: worst y {wy[0]} {wy[1][0]:.2e} / "
          f"{wy[1][1]:.2e}, worst a {wa[0]} {wa[2][0]:.2e} / {wa[2][1]:.2e}, heads {eh[0]:.2e} / {eh[1]:.2e}; native "
          f"{t1 - t0:.1f} s, layer oracle {time.perf_counter() - t1:.1f} s")
    assert len(rows) == 23
    if mode != "bf16":
        l2_bar, max_bar = LAYER_BARS[mode]
        for name, ey, ea in rows:
            assert ey[0] < l2_bar and ey[1] < max_bar, (name, "y", ey)
            assert ea[0] < l2_bar and ea[1] < max_bar, (name, "a", ea)
    assert max(eh) < HEAD_BARS[mode], eh


def check_layers(saved, sd32, mode, coord, B, dims, prob, reg, config):
    """saved[name] = (y, a, stats) as read from the arena, saved['cat'] / ['table'] / ['vw']: assert the statistics and (bf16)
    the rounding bars; -> ([(name, y (rel-L2, max), a (rel-L2, max))], heads (prob, reg) max error / maximum)"""
    def weight(key):
        w = sd32[key]
        return (w.bfloat16() if mode == "bf16" else w).double()      # bf16 mode: the packing rounds the weights to bf16

    dense = tr.scatter_dense(saved["vw"], coord, (B,) + tuple(dims)).permute(0, 4, 1, 2, 3)
    active = _active_sites(coord, B, dims)
    a_of = {}
    rows = []
    prev = None
    for name, spec in saved["table"]:
        y_k, a_k, st = saved[name]
        cv = "deconv" if spec.transposed else "conv"
        pre = f"middle_rpn.{name}"
        rm, rv = sd32[pre + ".batch_norm.running_mean"].double(), sd32[pre + ".batch_norm.running_var"].double()
        gamma, beta = sd32[pre + ".batch_norm.weight"].double(), sd32[pre + ".batch_norm.bias"].double()
        # statistics: [running_mean | 1/sqrt(running_var + eps) | gamma * invstd | beta]
        inv = 1.0 / torch.sqrt(rv + tr.BN_EPS)
        for i, want in enumerate((rm, inv, gamma * inv, beta)):
            assert float(((st[i] - want).abs() / want.abs().clamp(min=1e-30)).max()) < 1e-6, (name, i)
        # the executor's own input
        if name == "middle_layer.0":
            x = dense
        elif name in ("deconv1", "block2.0"):
            x = a_of["block1.4"]
        elif name in ("deconv2", "block3.0"):
            x = a_of["block2.5"]
        elif name == "block1.0":
            x = a_of["middle_layer.2"].reshape(B, 128, *a_of["middle_layer.2"].shape[3:])     # model.py:262: channel c*2+d
        else:
            x = prev
        bias = sd32[f"{pre}.{cv}.bias"].double()
        y64 = oracle_conv64(x, weight(f"{pre}.{cv}.weight"), spec, cv) + bias.view((1, -1) + (1,) * (x.dim() - 2))
        shp = (1, -1) + (1,) * (y64.dim() - 2)
        yk = _to_oracle(y_k, name, spec)
        ak = _to_oracle(a_k, name, spec)
        if name == "middle_layer.0":
            act = active[:, None].expand_as(y64)
            # the unwritten sites hold the bias as the flagged apply reads it (the stored dtype's value of the bias)
            yk_eff = torch.where(act, yk, (bias.float().bfloat16() if mode == "bf16" else bias.float()).double().view(shp))
            ycmp = (yk[act], y64[act])
        else:
            yk_eff = yk
            ycmp = (yk, y64)
        if mode == "bf16":
            assert_rounded(ycmp[0].float(), ycmp[1].numpy(), f"{config} {name} y")
            _, z = emulate_fp32_bn(yk_eff.float(), st[0].float().view(shp), st[2].float().view(shp), st[3].float().view(shp))
            assert_rounded(ak.float(), torch.relu(z).double().numpy(), f"{config} {name} a = relu(BN_running(y)) of its own y")
            ey, ea = _dist(*ycmp), _dist(ak, torch.relu(z).double())
        else:
            a64 = torch.relu((y64 - rm.view(shp)) * (gamma * inv).view(shp) + beta.view(shp))
            ey, ea = _dist(*ycmp), _dist(ak, a64)
        rows.append((name, ey, ea))
        a_of[name] = ak
        if not spec.transposed:
            prev = ak if name != "middle_layer.2" else ak.reshape(B, 128, *ak.shape[3:])
    # the heads from the concatenation: one 1x1 conv over 768 channels, sigmoid on the first two
    cat = rows_to_nchw64(saved["cat"], 2)
    hw = torch.cat([weight("middle_rpn.prob_conv.conv.weight"), weight("middle_rpn.reg_conv.conv.weight")], 0)
    hb = torch.cat([sd32["middle_rpn.prob_conv.conv.bias"], sd32["middle_rpn.reg_conv.conv.bias"]]).double()
    h = F.conv2d(cat, hw, hb)
    return rows, (rel_err(prob, torch.sigmoid(h[:, :2])), rel_err(reg, h[:, 2:]))


# ---- (e) the VFE in eval mode at production K -----------------------------------------------------------------------

def vfe_eval_float64(feature, sd, chunk=4096):
    """oracle/torch_ref.voxel_features(training=False) over chunks of voxels: with the running statistics every voxel is
    independent, so the chunks are exact (the (K,T,128) intermediates of K = 40k, T = 64 never exist at once)"""
    out = [tr.voxel_features(feature[i:i + chunk].double().cpu(), sd, False) for i in range(0, feature.shape[0], chunk)]
    return torch.cat(out, 0)


@pytest.mark.parametrize("config", ["car", "dense"])
def test_vfe_eval_at_production_K(config, request):
    """featnet_forward(training = False) — vn_vfe_fwd's eval route — with the foreign VFE statistics against float64
    voxel_features(training = False): car (K ~ 12.4k, T = 35) and dense (K ~ 40k, T = 64).  The running buffers are
    bit-unchanged afterwards."""
    from voxelnet_amd import model as M
    ctx, inp = request.getfixturevalue(f"{config}_eval"), request.getfixturevalue(f"{config}_inputs")
    m = _model(ctx["cls"], ctx["sd32"], "bf16", inp["grid"]).eval()
    fn = m.feature_net
    feature = torch.cat(inp["feats"], 0).contiguous()
    before = [b.clone() for b in fn._bufs()]
    vw, _, _ = M.featnet_forward(feature, [p.detach() for p in M._vfe_weights(fn)], fn._bufs(), False)
    torch.cuda.synchronize()
    ref = vfe_eval_float64(feature, ctx["sd"])
    e = rel_err(vw, ref)
    print(f"{config}: VFE eval, K = {feature.shape[0]}, T = {feature.shape[1]}: vs float64 {e:.2e}")
    assert e < 1e-4
    assert all(torch.equal(a, b) for a, b in zip(before, fn._bufs()))


# ---- (f) eval with gradients enabled: the per-layer route -----------------------------------------------------------

def test_car_eval_with_grad_enabled_maps(car_eval, car_inputs):  # noqa: F811
    """car B = 2, fp32: an eval detect with autograd on (a backward may follow) takes the per-layer orchestration, not the
    native executor; its maps are within the fp32 bar of the float64 oracle and within 1e-4 of the native eval maps"""
    from voxelnet_amd import _lib
    from voxelnet_amd import model as M
    inp = car_inputs
    try:
        native = native_eval("Car", inp, "fp32", car_eval["sd32"])
        m = _model("Car", car_eval["sd32"], "fp32", inp["grid"]).eval()
        called = []
        call = _lib.call
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(_lib, "call", lambda name, *a: (called.append(name), call(name, *a))[1])
            prob, reg = m.detect(inp["feats"], inp["coords"])
        torch.cuda.synchronize()
    finally:
        M.set_precision("bf16")
    assert prob.requires_grad and "vn_net_forward" not in called
    errs = _map_errors(prob.detach(), reg.detach(), car_eval["rp"], car_eval["rr"])
    en = (rel_err(prob.detach(), native[0]), rel_err(reg.detach(), native[1]))
    print(f"car fp32 eval with grad enabled: vs float64 {errs[0][0]:.2e} / {errs[0][1]:.2e}, vs the native eval maps "
          f"{en[0]:.2e} / {en[1]:.2e}")
    assert max(max(e) for e in errs) < MAP_BARS[("car", "fp32")], errs
    assert max(en) < 1e-4, en


# ---- (g) an eval forward leaves the model's state alone -------------------------------------------------------------

def _snapshot(m):
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def _assert_same(a, b, what):
    assert a.keys() == b.keys(), what
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k)


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_eval_forward_leaves_state_alone(car_eval, car_inputs, mode):  # noqa: F811
    """an eval detect changes no parameter, running statistic or num_batches_tracked, and two of them give bit-identical
    maps (the executor's cached prepare and arena pool carry nothing from one call to the next)"""
    from voxelnet_amd import model as M
    inp = car_inputs
    try:
        m = _model("Car", car_eval["sd32"], mode, inp["grid"]).eval()
        before = _snapshot(m)
        with torch.no_grad():
            p1, r1 = m.detect(inp["feats"], inp["coords"])
            p1, r1 = p1.clone(), r1.clone()
            p2, r2 = m.detect(inp["feats"], inp["coords"])
        torch.cuda.synchronize()
    finally:
        M.set_precision("bf16")
    _assert_same(before, _snapshot(m), "state after two eval forwards")
    assert torch.equal(p1, p2) and torch.equal(r1, r2)


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_train_validate_train_equals_train_train(car_eval, car_inputs, mode):  # noqa: F811
    """the reference's loop on one model: train_step(b0) -> model.eval(); detect of a B = 1 batch -> model.train();
    train_step(b2), against train_step(b0) -> train_step(b2) on a fresh identical model: outputs, gradients, parameters and
    running statistics bit-identical (the fused vn_net_step with ClipSGD both times).  The maps taken in between equal a
    fresh model's eval maps after loading the same state_dict, bit for bit."""
    from voxelnet_amd import model as M
    from voxelnet_amd.config import GRADIENT_CLIP, LR
    from voxelnet_amd.optim import ClipSGD
    inp, grid = car_inputs, car_inputs["grid"]
    f2, c2 = _frames(2, 2, grid, frame0=2)
    rng = np.random.default_rng(4242)

    def targets():
        pos = (rng.random((2, 200, 176, 2)) < 0.002).astype(np.float32)
        neg = ((rng.random((2, 200, 176, 2)) < 0.98) & (pos == 0)).astype(np.float32)
        tgt = (rng.standard_normal((2, 200, 176, 14)) * 0.1).astype(np.float32)
        return tuple(torch.from_numpy(a).to(DEV) for a in (pos, neg, tgt))
    batches = [((None, None, inp["feats"], None, inp["coords"], None, None), targets()),
               ((None, None, f2, None, c2, None, None), targets())]
    sd = tr.make_state_dict("Car")

    def run(validate):
        m = _model("Car", sd, mode, grid).train()
        opt = ClipSGD(list(m.parameters()), LR, GRADIENT_CLIP)
        outs, mid = [], None
        for i, (x, t) in enumerate(batches):
            if i == 1 and validate:
                m.eval()
                with torch.no_grad():
                    mid = [v.clone() for v in m.detect(inp["feats"][:1], inp["coords"][:1])]
                state = _snapshot(m)
                m.train()
            opt.zero_grad()
            assert m._step_fused_ok(mode, opt)
            outs.append([o.detach().clone() for o in m.train_step(x, DEV, opt, targets=t)])
        torch.cuda.synchronize()
        grads = {k: p.grad.detach().clone() for k, p in m.named_parameters()}
        return outs, grads, _snapshot(m), mid, (state if validate else None)
    try:
        o1, g1, s1, mid, state = run(True)
        o0, g0, s0, _, _ = run(False)
        fresh = _model("Car", state, mode, grid).eval()
        with torch.no_grad():
            want = fresh.detect(inp["feats"][:1], inp["coords"][:1])
        torch.cuda.synchronize()
    finally:
        M.set_precision("bf16")
    for a, b in zip(o1, o0):
        assert all(torch.equal(x, y) for x, y in zip(a, b)), "step outputs"
    _assert_same(g1, g0, "gradients")
    _assert_same(s1, s0, "parameters and running statistics")
    assert torch.equal(mid[0], want[0]) and torch.equal(mid[1], want[1]), "eval maps between the steps"
