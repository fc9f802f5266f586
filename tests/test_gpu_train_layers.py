"""GPU: the native executor's TRAIN-mode forward (RPN3D.detect in model.train(), csrc/runtime.hip vn_net_forward with
cfg.training = 1 — the forward of the benchmarked step), layer by layer, on the benchmarked configs: car B = 2, ped B = 2
and dense B = 4 in bf16, dense B = 4 in fp32 as well (its tiles are its own in every mode).

Why a test of its own.  The maps of the bf16 train step are held only loosely (0.12 .. 0.25: the ReLU/BatchNorm stack
amplifies bf16 rounding), the bf16 backward tests take the executor's saved forward as the truth, and the per-layer check
on the executor's own input (test_gpu_eval.py) runs in eval mode, which skips the routes only training takes: the batch
statistics the conv epilogues write into their slab rows, vn_bn_finalize_slab, the first layer's statistics with the
bias-filled sites, and the running-statistics update.  A few-percent error in one layer (one slab row of a statistic lost,
one tail tile stored wrong, one deconv slice of the concatenation misplaced) passed the suite.

What is checked, after the forward and before any backward, from the arena (vn_net_tensor_info on the training
configuration), for each of the 23 layers:
  * y against a float64 conv of the layer's own input (the previous layer's arena a, the bf16-valued weights in bf16 mode)
    plus bias: bf16 at half a bf16 ulp (test_gpu_bf16_parity.assert_rounded, no extra slack), fp32 at eval's LAYER_BARS.
    middle_layer.0 reads the executor's voxel rows (a gather per tap over the occupied voxels: exact, no dense grid); its y
    is compared wherever the plan writes it (only the active sites when the plan takes the list-based backward).
  * the statistics [mean | invstd | gamma * invstd | beta] against float64 statistics of the EXACT conv output y64 over all
    B*D*H*W sites (the epilogue sums the fp32 accumulator before the bf16 store: y64 is its reference; middle_layer.2 pools
    both depth slices of the BEV fold, middle_layer.0 counts the unreached sites at the bias).
  * a = relu(fmaf(S, y - mean, beta)) of the stored y with the arena statistics, everywhere (middle_layer.0's unreached sites
    at the stored bias).
  * the heads from the concatenation, and the 23 running statistics after the forward: 0.9 * init + 0.1 * (mean, unbiased
    var) from the same float64 statistics.
Bars beside their measured values below."""
import ctypes
import time

import pytest
import torch

from oracle import torch_ref as tr
from test_gpu_bf16_parity import EPS, assert_rounded, emulate_fp32_bn, oracle_conv64, rows_to_nchw64
from test_gpu_eval import HEAD_BARS, LAYER_BARS, _active_sites, _dist, _to_oracle
from test_gpu_native_chain import (DEV, MODES, arena_tensor, car_inputs, dense4_inputs,  # noqa: F401 (fixtures)
                                   ped_inputs, rel_err, tensor_info)

pytestmark = pytest.mark.gpu
CLASSES = {"car": "Car", "ped": "Pedestrian", "dense4": "Car"}
# the statistics against float64 (worst over the 23 layers and the configs of a mode): |mean - mean64| / std,
# |invstd * sqrt(var64 + eps) - 1|, |S / (gamma * invstd64) - 1|, running mean |rm - rm64| / std, running var |rv / rv64 - 1|
STAT_BARS = {"bf16": 5e-7,     # 1.7e-7 (ped block3.4 S)
             "fp32": 5e-7}     # 1.6e-7 (dense4 middle_layer.1 mean)


def native_train_forward(cls, inp, mode, keep):
    """model.train(); detect with autograd on, on the native executor with cfg.training == 1 (the forward of the train
    step).  keep(ws, cfg, K, m): called after the forward (the arena holds it).  -> (prob, reg, voxel rows as the VFE left
    them (fp32))"""
    from voxelnet_amd import _lib
    from voxelnet_amd import model as M
    M.set_precision(mode)
    m = M.RPN3D(cls)
    m.load_state_dict(tr.make_state_dict(cls))
    m.feature_net._grid = inp["grid"]
    m = m.to(DEV).train()
    assert m._native_ok(mode) and m.sparse_first_layer and m.training
    seen, cfgs, vws = [], [], []
    acquire, call, featnet_forward = M.RPN3D._ws_acquire, _lib.call, M.featnet_forward

    def spy(self, nbytes, device):
        ws = acquire(self, nbytes, device)
        seen.append((ws, nbytes))
        return ws

    def call_spy(name, *args):
        if name == "vn_net_forward":
            cfgs.append(_lib.VnNetConfig.from_buffer_copy(args[1]._obj))      # the configuration of the call, as passed
        return call(name, *args)

    def featnet_spy(*args):
        out = featnet_forward(*args)
        vws.append(out[0])
        return out
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(M.RPN3D, "_ws_acquire", spy)
        mp.setattr(_lib, "call", call_spy)
        mp.setattr(M, "featnet_forward", featnet_spy)
        prob, reg = m.detect(inp["feats"], inp["coords"])
    torch.cuda.synchronize()
    assert prob.requires_grad and len(seen) == 1 and len(cfgs) == 1 and len(vws) == 1, "the forward did not run on the native executor"
    assert cfgs[0].training == 1 and cfgs[0].sparse_first == 1 and cfgs[0].mode == MODES[mode], "not the train-mode executor"
    ws, nbytes = seen[0]
    D, H, W = inp["grid"].dims
    B, K = len(inp["feats"]), sum(int(f.shape[0]) for f in inp["feats"])
    cfg = _lib.VnNetConfig(B, D, H, W, m.middle_rpn._block1_stride, MODES[mode], 1, 1, 0, 0, 0, 0)
    assert all(getattr(cfg, f) == getattr(cfgs[0], f) for f in ("B", "D", "H", "W", "block1_stride", "grad_storage"))
    assert _lib.load().vn_net_workspace_bytes(ctypes.byref(cfg), K) == nbytes      # the plan the query walks is this one
    keep(ws, cfg, K, m)
    return prob.detach(), reg.detach(), vws[0].detach()


def first_layer64(vw64, coord, b, w64, spec, dims):
    """middle_layer.0 without its bias for sample b, channels last (D',H,W,64), float64: one gather per tap over the
    occupied voxels (the grid is zero everywhere else, so this is the dense conv3d exactly)"""
    od = spec.out_dims(dims)
    sel = coord[:, 0] == b
    c, x = coord[sel].long(), vw64[sel]
    out = torch.zeros((od[0] * od[1] * od[2], w64.shape[0]), dtype=torch.float64)
    for kd in range(spec.k[0]):
        for kh in range(spec.k[1]):
            for kw in range(spec.k[2]):
                # input site = output * stride - pad + tap  ->  output = (input + pad - tap) / stride
                n = [c[:, 1 + i] + spec.pad[i] - t for i, t in enumerate((kd, kh, kw))]
                ok = torch.ones(c.shape[0], dtype=torch.bool)
                o = []
                for i in range(3):
                    ok &= n[i] % spec.stride[i] == 0
                    o.append(torch.div(n[i], spec.stride[i], rounding_mode="floor"))
                    ok &= (o[i] >= 0) & (o[i] < od[i])
                idx = (o[0] * od[1] + o[1]) * od[2] + o[2]
                out.index_add_(0, idx[ok], x[ok] @ w64[:, :, kd, kh, kw].t())
    return out.view(tuple(od) + (w64.shape[0],))


def _source(name, prev):
    """the layer whose arena a is this layer's input"""
    if name in ("deconv1", "block2.0"):
        return "block1.4"
    if name in ("deconv2", "block3.0"):
        return "block2.5"
    return prev


def check_train_layers(tag, saved, sd, mode, inp, vw, prob, reg):
    """saved[name] = (y, a, stats) read from the arena after the train forward, saved['cat'] / ['table'] / ['running']
    (the model's running statistics after it): assert every bar; -> rows [(name, y err, a err, statistics err)]"""
    B, dims = len(inp["feats"]), inp["grid"].dims
    coord = torch.cat(inp["coords_cpu"], 0)
    K = coord.shape[0]
    bf16 = mode == "bf16"

    def weight(key):
        w = sd[key].float()
        return (w.bfloat16() if bf16 else w).double()      # bf16 mode: the packing rounds the weights to bf16
    vw64 = (vw.bfloat16().float() if bf16 else vw).double().cpu()       # the rows the rulebook reads (vn_cast_rows: RNE)
    active = _active_sites(coord, B, dims)
    # the plan's first-layer route (csrc/runtime.hip make_plan: list_bwd needs min(18 K, M0) * 10 <= 3 M0): with the
    # list-based backward nothing reads y at the unreached sites and the bias fill is skipped; the dense route writes it
    M0 = active.numel()
    y_dense = min(18 * K, M0) * 10 > M0 * 3
    assert y_dense == (not tag.startswith("car")), (tag, K, M0)      # car B = 2: the list route; ped and dense B = 4: dense
    rows = []
    prev = None
    for name, spec in saved["table"]:
        y_k, a_k, st = saved[name]
        st = st.reshape(4, spec.cout).double().cpu()
        cv = "deconv" if spec.transposed else "conv"
        pre = f"middle_rpn.{name}"
        bias = sd[f"{pre}.{cv}.bias"].double()
        gamma, beta = sd[pre + ".batch_norm.weight"].double(), sd[pre + ".batch_norm.bias"].double()
        w64 = weight(f"{pre}.{cv}.weight")
        sf = [st[i].float() for i in range(4)]
        s1 = torch.zeros(spec.cout, dtype=torch.float64)        # sums of y64 - bias and of its square over every site
        s2 = torch.zeros(spec.cout, dtype=torch.float64)
        n = 0
        ey, ea = (0.0, 0.0), (0.0, 0.0)
        for b in range(B):           # one sample at a time: the dense B = 4 first layer is 2.9 GB in float64
            if name == "middle_layer.0":
                c64 = first_layer64(vw64, coord, b, w64, spec, dims)             # (D',H,W,64), channels last
                y64 = c64 + bias
                yk = y_k[b].double().cpu()
                ak = a_k[b].double().cpu()
                act = active[b][..., None].expand_as(y64)
                ycmp = (yk, y64) if y_dense else (yk[act], y64[act])
                # the unreached sites as the flagged apply reads them: the stored dtype's value of the bias
                yk_eff = torch.where(act, yk, (bias.float().bfloat16() if bf16 else bias.float()).double())
                _, z = emulate_fp32_bn(yk_eff.float(), sf[0], sf[2], sf[3])
                c64 = c64.reshape(-1, spec.cout)
                red = 0
            else:
                src = _source(name, prev)
                x = _to_oracle(saved[src][1][b:b + 1], src, dict(saved["table"])[src])
                if src == "middle_layer.2":
                    x = x.reshape(1, 128, *x.shape[3:])          # the BEV fold (model.py:262): channel c*2 + d
                shp = (1, -1) + (1,) * (x.dim() - 2)
                c64 = oracle_conv64(x, w64, spec, cv)
                y64 = c64 + bias.view(shp)
                yk, ak = _to_oracle(y_k[b:b + 1], name, spec), _to_oracle(a_k[b:b + 1], name, spec)
                ycmp = (yk, y64)
                _, z = emulate_fp32_bn(yk.float(), *(sf[i].view(shp) for i in (0, 2, 3)))
                red = [0] + list(range(2, c64.dim()))
            aref = torch.relu(z).double()
            if bf16:
                e1 = assert_rounded(ycmp[0].float(), ycmp[1].numpy(), f"{tag} {name} y (sample {b})")
                e2 = assert_rounded(ak.float(), aref.numpy(), f"{tag} {name} a = relu(BN(y)) of its own y (sample {b})")
                e1, e2 = (e1[1], e1[0]), (e2[1], e2[0])
            else:
                e1, e2 = _dist(*ycmp), _dist(ak, aref)
            ey, ea = tuple(map(max, ey, e1)), tuple(map(max, ea, e2))
            s1 += c64.sum(dim=red)
            s2 += (c64 * c64).sum(dim=red)
            n += c64.numel() // spec.cout
        assert n == y_k.numel() // spec.cout, name
        # ---- the batch statistics, against float64 statistics of the exact conv output
        mc = s1 / n
        var = s2 / n - mc * mc
        mean, std = bias + mc, var.sqrt()
        inv = 1.0 / (var + EPS).sqrt()
        rm0, rv0 = sd[pre + ".batch_norm.running_mean"].double(), sd[pre + ".batch_norm.running_var"].double()
        rm, rv = saved["running"][name]
        es = (float(((st[0] - mean).abs() / std).max()),
              float((st[1] / inv - 1).abs().max()),
              float((st[2] / (gamma * inv) - 1).abs().max()),
              float(((rm - (0.9 * rm0 + 0.1 * mean)).abs() / std).max()),
              float((rv / (0.9 * rv0 + 0.1 * var * n / (n - 1)) - 1).abs().max()))
        assert float(((st[3] - beta).abs() / beta.abs().clamp(min=1e-30)).max()) < 1e-6, (tag, name, "beta")
        rows.append((name, ey, ea, es))
        if mode != "bf16":
            l2_bar, max_bar = LAYER_BARS[mode]
            assert ey[0] < l2_bar and ey[1] < max_bar, (tag, name, "y", ey)
            assert ea[0] < l2_bar and ea[1] < max_bar, (tag, name, "a", ea)
        assert max(es) < STAT_BARS[mode], (tag, name, "mean, invstd, gamma*invstd, running mean, running var", es)
        if not spec.transposed:
            prev = name
    # ---- the heads from the concatenation: one 1x1 conv over 768 channels, sigmoid on the first two
    cat = rows_to_nchw64(saved["cat"], 2)
    hw = torch.cat([weight("middle_rpn.prob_conv.conv.weight"), weight("middle_rpn.reg_conv.conv.weight")], 0)
    hb = torch.cat([sd["middle_rpn.prob_conv.conv.bias"], sd["middle_rpn.reg_conv.conv.bias"]]).double()
    h = torch.nn.functional.conv2d(cat, hw, hb)
    eh = (rel_err(prob, torch.sigmoid(h[:, :2])), rel_err(reg, h[:, 2:]))
    assert max(eh) < HEAD_BARS[mode], (tag, eh)
    return rows, eh


@pytest.mark.parametrize("config,mode", [("car", "bf16"), ("ped", "bf16"), ("dense4", "bf16"), ("dense4", "fp32")])
def test_native_train_layers_vs_float64_on_own_input(config, mode, request):
    from voxelnet_amd import _lib
    from voxelnet_amd import model as M
    from voxelnet_amd import net as N
    inp = request.getfixturevalue(f"{config}_inputs")
    cls = CLASSES[config]
    saved = {}

    def keep(ws, cfg, K, m):
        table = N.layer_table(m.middle_rpn._block1_stride)
        assert len(table) == 23
        for l, (name, spec) in enumerate(table):
            saved[name] = (arena_tensor(ws, tensor_info(cfg, K, l, _lib.VN_NET_Y)),
                           arena_tensor(ws, tensor_info(cfg, K, l, _lib.VN_NET_A)),
                           arena_tensor(ws, tensor_info(cfg, K, l, _lib.VN_NET_STATS)))
        saved["cat"] = arena_tensor(ws, tensor_info(cfg, K, len(table) - 1, _lib.VN_NET_A), C=768)
        saved["table"] = table
        state = m.state_dict()
        saved["running"] = {name: tuple(state[f"middle_rpn.{name}.batch_norm.running_{s}"].double().cpu() for s in ("mean", "var"))
                            for name, _ in table}
    t0 = time.perf_counter()
    try:
        prob, reg, vw = native_train_forward(cls, inp, mode, keep)
    finally:
        M.set_precision("bf16")
    t1 = time.perf_counter()
    tag = f"{config} {mode}"
    rows, eh = check_train_layers(tag, saved, tr.make_state_dict(cls), mode, inp, vw, prob, reg)
    for name, ey, ea, es in rows:
        print(f"   {tag} {name:16s} y rel-L2 {ey[0]:.2e} max {ey[1]:.2e} | a rel-L2 {ea[0]:.2e} max {ea[1]:.2e} | stats "
              + " ".join(f"{e:.1e}" for e in es))
    wy = max(rows, key=lambda r: r[1][0])
    wa = max(rows, key=lambda r: r[2][0])
    ws_ = [max(rows, key=lambda r: r[3][i]) for i in range(5)]
    print(f"{tag} train layers vs float64 on the executor's own input: worst y {wy[0]} rel-L2 {wy[1][0]:.2e} / max "
          f"{wy[1][1]:.2e}, worst a {wa[0]} {wa[2][0]:.2e} / {wa[2][1]:.2e}; statistics (mean, invstd, S, running mean, "
          f"running var) " + ", ".join(f"{r[0]} {r[3][i]:.1e}" for i, r in enumerate(ws_)) +
          f"; heads {eh[0]:.2e} / {eh[1]:.2e}; native {t1 - t0:.1f} s, oracle {time.perf_counter() - t1:.1f} s")
    assert len(rows) == 23
