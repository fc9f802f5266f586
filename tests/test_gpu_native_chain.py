"""GPU: the native executor's gradients (csrc/runtime.hip: vn_net_forward / vn_net_backward, the calls RPN3D.detect and
the benchmarked RPN3D.train_step make) at FULL size against a float64 oracle evaluated with the executor's own ReLU
decisions.

Why frozen masks.  One ReLU-mask element flipped by rounding (z within an ulp of 0) moves every upstream gradient by
1e-2 .. 1e-1, which is why the unmasked full-size checks (test_gpu_model.test_car_full_backward,
test_gpu_configs.test_dense_config_fp32_step_vs_oracle) can only hold the chained gradients to 0.1.  Here the oracle
(oracle/torch_ref.forward_backward(masks=...)) multiplies by the masks the executor's forward computed, so what is left is
arithmetic: a wrong term on any executor-only route — the first layer's BatchNorm backward from the active sites
(list_bwd), middle_layer.1's weight gradient from the active sites plus a rank-1 term (sparse_w1), fp32x3 middle_layer.2's
weight gradient as three in-place bf16 passes (m2_passes), the weight-gradient unpack on the side stream, the fused
BatchNorm-backward epilogues, the dense first-layer route of the dense config, the ped plans (block1 at stride 1) — shows
up as an order-of-magnitude outlier in one parameter's gradient.

The masks are read from the executor's workspace arena: RPN3D._ws_acquire is wrapped (same call sequence) to get the
arena, vn_net_tensor_info says where each layer's activation is, and they are read after the forward, before backward().

Bars: relative L2 of every gradient, max error / map maximum for the maps, per config and mode in BARS (measured values
beside them).  bf16: the native gradients against an EXACT fp32 chain through the executor's own saved forward, the VFE
gradients included, at test_gpu_bf16_parity's FROZEN_L2 / FROZEN_COS.  Measured worst: middle_layer.0.batch_norm.bias
0.0495 / cos 0.99877 (the per-layer bf16 chain through the same forward: 0.0531 / 0.99859 — the bf16 rounding of a sum
that nearly cancels, not an executor route); every other gradient <= 0.020, cos >= 0.9998.  The same for ped B = 2 (worst
middle_layer.0.batch_norm.bias 0.033 / 0.99948) and dense B = 4 (middle_layer.1.batch_norm.bias 0.037 / 0.99939).  The
forward those chains start from is checked layer by layer in tests/test_gpu_train_layers.py."""
import ctypes
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import torch_ref as tr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = {"bf16": 0, "fp32": 1, "fp32x3": 2}
# (map bar, gradient bar) per config and mode: about 3x the measured worst (in the comments: maps prob / reg, worst
# gradient), below the ceilings of maps 1e-4 / gradients 2e-3 (fp32) and 1e-3 / 5e-3 (fp32x3)
BARS = {
    ("car", "fp32"): (5e-5, 4e-4),       # 1.4e-5 / 7.1e-6, middle_layer.2.conv.weight 1.2e-4
    ("car", "fp32x3"): (4e-4, 5e-4),     # 1.3e-4 / 7.8e-5, deconv3.deconv.weight 1.7e-4
    ("ped", "fp32"): (5e-5, 2e-4),       # 1.4e-5 / 6.4e-6, middle_layer.1.conv.weight 6.3e-5
    ("ped", "fp32x3"): (5e-4, 6e-4),     # 1.6e-4 / 6.8e-5, block3.5.batch_norm.weight 1.8e-4
    ("dense", "fp32"): (4e-5, 1.5e-4),   # 1.1e-5 / 7.6e-6, middle_layer.1.conv.weight 4.2e-5
    ("dense", "fp32x3"): (4e-4, 7e-4),   # 1.2e-4 / 7.1e-5, block3.5.batch_norm.weight 2.1e-4
}


def state_dict_f64(cls):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in tr.make_state_dict(cls).items()}


def dead_bias(k):
    """a conv / deconv bias in front of a train-mode BatchNorm: its gradient is identically 0"""
    return (k.endswith("conv.bias") and "prob_conv" not in k and "reg_conv" not in k) or k.endswith("deconv.bias")


def rel_err(a, b):
    return float((a.double().cpu() - b.double().cpu()).abs().max() / b.double().abs().max().clamp(min=1e-30))


# ---- the executor's arena -------------------------------------------------------------------------------------------

def tensor_info(cfg, K, layer, which):
    from voxelnet_amd import _lib
    info = _lib.VnNetTensorInfo()
    _lib.call("vn_net_tensor_info", ctypes.byref(cfg), K, layer, which, ctypes.byref(info))
    return info


def arena_tensor(ws, info, C=None):
    """the region vn_net_tensor_info describes as a fresh (B,D,H,W,C) fp32 tensor (bf16 widened, VN_F32X3S: hi + lo).
    C: read more channels than the region's own (the deconvs' slices of the concatenation: the whole 768)"""
    from voxelnet_amd import _lib
    from test_gpu_x3_split import unsplit
    C = info.C if C is None else C
    esz = 2 if info.dtype == _lib.VN_BF16 else 4
    n = (info.B - 1) * info.sB + (info.D - 1) * info.sD + (info.H - 1) * info.sH + (info.W - 1) * info.sW + C
    assert info.offset % 256 == 0 and info.offset + n * esz <= ws.numel()
    raw = ws[info.offset:info.offset + n * esz].view(torch.bfloat16 if esz == 2 else torch.float32)
    t = raw.as_strided((info.B, info.D, info.H, info.W, C), (info.sB, info.sD, info.sH, info.sW, 1))
    out = torch.empty(t.shape, dtype=torch.float32, device=ws.device).copy_(t)
    if info.dtype == _lib.VN_F32X3S:
        hi, lo = unsplit(out)
        out = hi + lo
    return out


def arena_masks(ws, cfg, K, table):
    """ReLU decisions of the executor's forward, per layer, in the oracle's NC(D)HW output shapes (bool, host)"""
    from voxelnet_amd import _lib
    out = {}
    for l, (name, spec) in enumerate(table):
        a = arena_tensor(ws, tensor_info(cfg, K, l, _lib.VN_NET_A))
        B = a.shape[0]
        if name == "middle_layer.2":                 # BEV rows (B,1,H,W,128), channel d*64 + c  ->  (B,64,2,H,W)
            m = a.reshape(B, a.shape[2], a.shape[3], 2, 64).permute(0, 4, 3, 1, 2)
        elif spec.dim == 3:
            m = a.permute(0, 4, 1, 2, 3)
        else:
            m = a[:, 0].permute(0, 3, 1, 2)
        out[name] = (m > 0).cpu().contiguous()
    return out


def native_run(cls, feats, coords, mode, dp, dr, grid=None, sd=None, keep=None):
    """train-mode forward through the native executor (sparse first layer, as in production), the ReLU masks read from
    its arena, then backward() with dp / dr.  keep(ws, cfg, K, m): called between forward and backward (the arena holds the
    forward).  -> (prob, reg, {name: grad} (float64, host), masks)"""
    from voxelnet_amd import _lib
    from voxelnet_amd import model as M
    from voxelnet_amd import net as N
    M.set_precision(mode)
    m = M.RPN3D(cls)
    m.load_state_dict(sd if sd is not None else tr.make_state_dict(cls))
    if grid is not None:
        m.feature_net._grid = grid
    m = m.to(DEV).train()
    assert m._native_ok(mode) and m.sparse_first_layer and m.training
    seen = []
    acquire = M.RPN3D._ws_acquire

    def spy(self, nbytes, device):
        ws = acquire(self, nbytes, device)
        seen.append((ws, nbytes))
        return ws
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(M.RPN3D, "_ws_acquire", spy)
        prob, reg = m.detect(feats, coords)
    assert len(seen) == 1, "the forward did not run on the native executor"
    torch.cuda.synchronize()
    ws, nbytes = seen[0]
    D, H, W = m.feature_net._grid.dims
    B, K = len(feats), sum(int(f.shape[0]) for f in feats)
    cfg = _lib.VnNetConfig(B, D, H, W, m.middle_rpn._block1_stride, MODES[mode], 1, 1, 0, 0, 0, 0)
    assert _lib.load().vn_net_workspace_bytes(ctypes.byref(cfg), K) == nbytes      # the plan the query walks is this one
    table = N.layer_table(m.middle_rpn._block1_stride)
    masks = arena_masks(ws, cfg, K, table)
    if keep is not None:
        keep(ws, cfg, K, m)
    torch.autograd.backward([prob, reg], [dp.to(DEV), dr.to(DEV)])
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().double().cpu() for k, p in m.named_parameters()}
    return prob.detach(), reg.detach(), grads, masks


def compare(tag, prob, reg, grads, rp, rr, ref, map_bar, grad_bar):
    ep, er = rel_err(prob, rp), rel_err(reg, rr)
    rows = []
    for k, g in grads.items():
        if dead_bias(k):
            assert float(g.abs().max()) == 0.0, (tag, k)
            continue
        r = ref[k].double()
        rows.append((k, float((g - r).norm() / (r.norm() + 1e-30)), float((g - r).abs().max() / r.abs().max().clamp(min=1e-30))))
    for k, l2, mx in rows:
        print(f"   {tag} {k:52s} rel-L2 {l2:.2e}  max err {mx:.2e}")
    worst = max(rows, key=lambda r: r[1])
    print(f"{tag}: maps prob {ep:.2e} reg {er:.2e} (bar {map_bar:.0e}); worst gradient {worst[0]} rel-L2 {worst[1]:.2e} "
          f"(bar {grad_bar:.0e}); {len(rows)} gradients + {len(grads) - len(rows)} dead biases")
    assert len(grads) == 104
    assert ep < map_bar and er < map_bar, (tag, ep, er)
    assert worst[1] < grad_bar, (tag, worst)


# ---- inputs ---------------------------------------------------------------------------------------------------------

def _voxelized(config_id, batch, grid, seed):
    from voxelnet_amd import synth
    from voxelnet_amd.voxelize import voxelize_device
    feats, coords = [], []
    for b, f in enumerate(synth.workload_frames(config_id, batch=batch)):
        fb, cb, _ = voxelize_device(torch.from_numpy(f).to(DEV), grid, b, coord_cols=4)
        feats.append(fb)
        coords.append(cb)
    h, w = grid.H // grid.block1_stride, grid.W // grid.block1_stride
    rng = np.random.default_rng(seed)
    dp = torch.from_numpy((rng.standard_normal((batch, 2, h, w)) * 1e-2).astype(np.float32))
    dr = torch.from_numpy((rng.standard_normal((batch, 14, h, w)) * 1e-2).astype(np.float32))
    return dict(feats=feats, coords=coords, dp=dp, dr=dr, grid=grid,
                feats64=[f.cpu().double() for f in feats], coords_cpu=[c.cpu() for c in coords])


@pytest.fixture(scope="module")
def car_inputs():
    from voxelnet_amd.config import grid_config
    grid = grid_config("Car")
    assert grid.dims == (10, 400, 352) and grid.block1_stride == 2
    return _voxelized(2, 2, grid, 77)            # bench.py's frames: BASELINE configs[1], B = 2


@pytest.fixture(scope="module")
def ped_inputs():
    from voxelnet_amd.config import grid_config
    grid = grid_config("Pedestrian")
    assert grid.dims == (10, 200, 240) and grid.block1_stride == 1
    return _voxelized(3, 2, grid, 3300)          # BASELINE configs[2], B = 2


@pytest.fixture(scope="module")
def dense_inputs():
    from voxelnet_amd.config import grid_config
    grid = grid_config("Car", T=64)
    return _voxelized(5, 1, grid, 78)            # BASELINE configs[4] at B = 1 (~40k voxels, T = 64)


@pytest.fixture(scope="module")
def dense4_inputs():
    from voxelnet_amd.config import grid_config
    grid = grid_config("Car", T=64)
    return _voxelized(5, 4, grid, 79)            # BASELINE configs[4] at its benchmarked B = 4 (~160k voxels)


def _masked_oracle_check(tag, cls, inp, mode):
    from voxelnet_amd import model as M
    t0 = time.perf_counter()
    try:
        prob, reg, grads, masks = native_run(cls, inp["feats"], inp["coords"], mode, inp["dp"], inp["dr"], grid=inp["grid"])
    finally:
        M.set_precision("bf16")
    t1 = time.perf_counter()
    torch.cuda.empty_cache()
    rp, rr, ref = tr.forward_backward(inp["feats64"], inp["coords_cpu"], state_dict_f64(cls), inp["grid"].dims, cls,
                                      inp["dp"].double(), inp["dr"].double(), masks=masks)
    t2 = time.perf_counter()
    print(f"{tag}: native step {t1 - t0:.1f} s, float64 oracle {t2 - t1:.1f} s")
    compare(tag, prob, reg, grads, rp, rr, ref, *BARS[tuple(tag.split()[:2])])


@pytest.mark.parametrize("mode", ["fp32", "fp32x3"])
def test_car_batch2_native_gradients_vs_float64_with_frozen_masks(car_inputs, mode):
    """(a) the benchmark's shape: car grid 10 x 400 x 352, B = 2, bench frames — the sparse first-layer routes (list_bwd,
    sparse_w1) and, in fp32x3, middle_layer.2's three-pass weight gradient"""
    _masked_oracle_check(f"car {mode}", "Car", car_inputs, mode)


@pytest.mark.parametrize("mode", ["fp32", "fp32x3"])
def test_ped_batch2_native_gradients_vs_float64_with_frozen_masks(ped_inputs, mode):
    """(b) ped grid 10 x 200 x 240, B = 2: block1 at stride 1 (200 x 240 maps at 128 channels)"""
    _masked_oracle_check(f"ped {mode}", "Pedestrian", ped_inputs, mode)


@pytest.mark.parametrize("mode", ["fp32", "fp32x3"])
def test_dense_batch1_native_gradients_vs_float64_with_frozen_masks(dense_inputs, mode):
    """(c) dense config, B = 1: at ~40k voxels the plan leaves the first layer's sparse backward routes (csrc/runtime.hip
    make_plan: list_bwd needs acap * 10 <= M0 * 3, acap = min(18 K, M0)) — the dense first-layer route"""
    K = sum(int(f.shape[0]) for f in dense_inputs["feats"])
    D, H, W = dense_inputs["grid"].dims
    M0 = 1 * ((D + 2 - 3) // 2 + 1) * H * W
    assert min(18 * K, M0) * 10 > M0 * 3, K
    _masked_oracle_check(f"dense {mode}", "Car", dense_inputs, mode)


def test_bf16_native_gradients_vs_exact_chain_on_the_native_forward(car_inputs):
    """(d) the benchmarked bf16 mode, car B = 2: the native bf16 gradients against an EXACT fp32 backward chain (per-layer
    orchestration, net.middle_backward + model.featnet_backward, fp32 kernels and storage) through the executor's own saved
    forward — its y / a / statistics read from the arena and widened to fp32 — so both see the same ReLU masks and
    normalised values and differ only in what the bf16 backward rounds.  The VFE gradients included: the stable VFE check
    the bf16-vs-fp32 step comparison (test_bf16_step_vs_fp32_step, forward-induced chaos) cannot give."""
    from test_gpu_bf16_parity import FROZEN_COS, FROZEN_L2
    rows = _bf16_exact_chain("car", "Car", car_inputs)
    for k, l2, cos, pl2, pcos, nl2, _ in rows:
        assert l2 < FROZEN_L2, (k, l2, cos)
        # the cosine bar holds unless the per-layer bf16 chain through the same forward misses it too (then it is the
        # rounding of the bf16 backward itself, not an executor route): the executor may not be further off than it
        assert cos > FROZEN_COS or (pcos <= FROZEN_COS and l2 <= 1.25 * pl2), (k, l2, cos, pl2, pcos)


@pytest.mark.parametrize("config", ["ped", "dense4"])
def test_bf16_native_gradients_vs_exact_chain_on_the_other_benchmarked_configs(config, request):
    """(e) as (d) for the other two benchmarked bf16 steps: ped B = 2 (block1 at stride 1) and dense B = 4 (the dense
    first-layer route, the batch-4 tiles).  A gradient may miss a bar only where the per-layer bf16 chain through the same
    forward misses it too — the rounding of the bf16 backward itself, not an executor route — and the executor is then
    within 1.25x of that chain."""
    from test_gpu_bf16_parity import FROZEN_COS, FROZEN_L2
    rows = _bf16_exact_chain(config, {"ped": "Pedestrian", "dense4": "Car"}[config], request.getfixturevalue(f"{config}_inputs"))
    for k, l2, cos, pl2, pcos, nl2, _ in rows:
        assert l2 < FROZEN_L2 or (pl2 >= FROZEN_L2 and l2 <= 1.25 * pl2), (config, k, l2, cos, pl2, pcos)
        assert cos > FROZEN_COS or (pcos <= FROZEN_COS and l2 <= 1.25 * pl2), (config, k, l2, cos, pl2, pcos)


def _bf16_exact_chain(tag, cls, inp):
    """the native bf16 step's gradients and the two chains through its saved forward (test (d)); prints the table ->
    [(parameter, native vs exact rel-L2, cos, per-layer bf16 vs exact rel-L2, cos, native vs per-layer rel-L2, cos)]"""
    from test_gpu_bf16_parity import FROZEN_COS, FROZEN_L2, _bf16_valued
    from voxelnet_amd import _lib
    from voxelnet_amd import engine as E
    from voxelnet_amd import model as M
    from voxelnet_amd import net as N
    from voxelnet_amd.engine import Rows
    t0 = time.perf_counter()
    sd = _bf16_valued(tr.make_state_dict(cls))
    saved = {}

    def keep(ws, cfg, K, m):
        table = N.layer_table(m.middle_rpn._block1_stride)
        for l, (name, spec) in enumerate(table):
            y = arena_tensor(ws, tensor_info(cfg, K, l, _lib.VN_NET_Y))
            st = arena_tensor(ws, tensor_info(cfg, K, l, _lib.VN_NET_STATS)).reshape(-1).contiguous()
            assert st.numel() == 4 * spec.cout
            saved[name] = (spec, y, arena_tensor(ws, tensor_info(cfg, K, l, _lib.VN_NET_A)), st)
        d3 = tensor_info(cfg, K, len(table) - 1, _lib.VN_NET_A)
        assert d3.C == 256 and d3.sW == 768
        saved["cat"] = arena_tensor(ws, d3, C=768)
        saved["table"] = table
    try:
        prob, reg, nat, _ = native_run(cls, inp["feats"], inp["coords"], "bf16", inp["dp"], inp["dr"], grid=inp["grid"], sd=sd,
                                       keep=keep)
        # the same module state for the exact chain (weights rounded to bf16 values: what the bf16 packing reads)
        m = M.RPN3D(cls)
        m.load_state_dict(sd)
        m.feature_net._grid = inp["grid"]
        m = m.to(DEV).train()
        fn, mid = m.feature_net, m.middle_rpn
        feature = torch.cat(inp["feats"], 0).contiguous()
        coord = torch.cat(inp["coords"], 0).contiguous()
        B = len(inp["feats"])
        vparams = [p.detach() for p in M._vfe_weights(fn)]
        names, P, Bf, flat = M._collect_middle(mid)
        P = M._detached(P)
        P["heads"] = M._heads_params([f.detach() for f in flat[-4:]])
        vw, stats, wst = M.featnet_forward(feature, vparams, fn._bufs(), True)
        vw_rows = vw.bfloat16()
        # middle_layer.0's y: the executor writes it only at the active sites (an occupied voxel within the 3x3x3
        # window); everywhere else the layer's output is its bias
        D, H, W = inp["grid"].dims
        c = coord.long().cpu()
        occ = torch.zeros((B, 1, D, H, W), dtype=torch.float32)
        occ[c[:, 0], 0, c[:, 1], c[:, 2], c[:, 3]] = 1.0
        active = (F.conv3d(occ, torch.ones((1, 1, 3, 3, 3)), stride=(2, 1, 1), padding=1)[:, 0] > 0).to(DEV)
        spec0, y0, a0, st0 = saved["middle_layer.0"]
        y0 = torch.where(active[..., None], y0, P["middle_layer.0"]["bias"].view(1, 1, 1, 1, -1))
        saved["middle_layer.0"] = (spec0, y0, a0, st0)
        hf, wf = prob.shape[2], prob.shape[3]
        cat_off = {"deconv3": 0, "deconv2": 256, "deconv1": 512}

        def frozen_state(mode, dt):
            # the executor's forward as per-layer orchestration state: each layer's input is the previous layer's a (the BEV
            # a of middle_layer.2 for block1.0, the last a of the block before for block2.0 / deconv1 and block3.0 / deconv2)
            st = N.MiddleState()
            st.layers, st.block1_stride, st.mode, st.x3 = {}, mid._block1_stride, mode, False
            st.prob, st.fmap, st.sparse = prob, (hf, wf), (coord, vw_rows.to(dt))
            cat = saved["cat"].to(dt)
            prev = None
            for name, spec in saved["table"]:
                _, y, a, stt = saved[name]
                if name in ("deconv1", "block2.0"):
                    src = saved["block1.4"][2]
                elif name in ("deconv2", "block3.0"):
                    src = saved["block2.5"][2]
                else:
                    src = prev
                t = E.LayerState()
                t.spec, t.stats, t.x3 = spec, stt, False
                t.x = Rows(src.to(dt), src.shape[-1]) if src is not None else None
                t.in_dims = tuple(src.shape[1:4]) if src is not None else (D, H, W)
                t.out_dims = tuple(y.shape[1:4])
                t.y = Rows(y.to(dt), spec.cout)
                t.a = Rows(cat[..., cat_off[name]:cat_off[name] + 256], 256) if spec.transposed else Rows(a.to(dt), a.shape[-1])
                st.layers[name] = t
                if not spec.transposed:
                    prev = a
            th = E.LayerState()
            th.spec, th.stats, th.x3, th.a = N.HEADS, None, False, None
            th.x = Rows(cat, 768)
            th.y = Rows(torch.empty((B, 1, hf, wf, 16), dtype=torch.float32, device=DEV), 16)
            th.in_dims = th.out_dims = (1, hf, wf)
            st.layers["heads"] = th
            G, dvw = N.middle_backward(st, inp["dp"].to(DEV), inp["dr"].to(DEV), P)
            return G, M.featnet_backward(feature, wst, stats, dvw, vparams)
        # the exact chain, and (to tell the executor's routes from the bf16 rounding of the backward itself) the per-layer
        # bf16 chain through the same forward
        Gf, vg_f = frozen_state("fp32", torch.float32)
        Gb, vg_b = frozen_state("bf16", torch.bfloat16)
        torch.cuda.synchronize()
    finally:
        M.set_precision("bf16")
    def flat(G, vg):
        out = {}
        for n in names:
            cv = "deconv" if n.startswith("deconv") else "conv"
            out[f"middle_rpn.{n}.{cv}.weight"] = G[n]["weight"]
            out[f"middle_rpn.{n}.batch_norm.weight"] = G[n]["gamma"]
            out[f"middle_rpn.{n}.batch_norm.bias"] = G[n]["beta"]
        out["middle_rpn.prob_conv.conv.weight"], out["middle_rpn.reg_conv.conv.weight"] = G["heads"]["weight"][:2], G["heads"]["weight"][2:]
        out["middle_rpn.prob_conv.conv.bias"], out["middle_rpn.reg_conv.conv.bias"] = G["heads"]["bias"][:2], G["heads"]["bias"][2:]
        for key, g in zip(M.VFE_KEYS, vg):
            out[key] = g
        return {k: v.double().cpu() for k, v in out.items()}

    def dist(a, b):
        b = b.reshape(a.shape)
        return float((a - b).norm() / (b.norm() + 1e-30)), float((a * b).sum() / (a.norm() * b.norm() + 1e-30))
    exact, layered = flat(Gf, vg_f), flat(Gb, vg_b)
    rows = []
    for k, g in nat.items():
        if dead_bias(k):
            assert float(g.abs().max()) == 0.0, k
            continue
        rows.append((k,) + dist(g, exact[k]) + dist(layered[k], exact[k]) + dist(g, layered[k]))
    for k, l2, cos, pl2, pcos, nl2, _ in rows:
        print(f"   {tag} bf16 vs exact chain on the native forward: {k:52s} native rel-L2 {l2:.4f} cos {cos:.5f} | "
              f"per-layer bf16 {pl2:.4f} {pcos:.5f} | native vs per-layer {nl2:.4f}")
    worst = max(rows, key=lambda r: r[1])
    wcos = min(rows, key=lambda r: r[2])
    print(f"{tag} bf16 native vs exact chain: worst {worst[:3]}, lowest cosine {wcos[:3]} ({len(rows)} gradients; bars "
          f"{FROZEN_L2} / {FROZEN_COS}); {time.perf_counter() - t0:.1f} s")
    assert len(rows) + sum(map(dead_bias, nat)) == 104
    return rows
