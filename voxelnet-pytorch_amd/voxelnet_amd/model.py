"""nn.Module surface of the reference's hot path, backed by libvoxelnet_hip.so.

Same class names, constructor arguments, attribute names (=> state_dict keys) and
forward signatures as /root/reference/voxelnet/model.py:
  VFELayer            model.py:60-82     (parameter container; see note)
  FeatureLearningNet  model.py:85-108
  ConvMD              model.py:111-167
  DeConv2d            model.py:170-199
  MiddleConvNet       model.py:202-281
  RPN3D               model.py:284-362   (forward + loss; predict/NMS are out of scope)
so `model(data, device); loss.backward(); clip_grad_norm_; SGD.step()` (train.py:148-155)
runs unchanged.  The nn.Linear / nn.Conv* / nn.BatchNorm* sub-modules only HOLD the
parameters and buffers (identical init and state_dict keys); their ATen forwards are
never called — every forward/backward goes through the C ABI via the
torch.autograd.Functions below.  There is no CPU path: CPU tensors raise.
"""
import contextlib
import ctypes
import math
import os

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from . import engine as E
from . import net as N
from .config import ALPHA, BETA, SIGMA, grid_config
from .engine import Rows

_PRECISION = {"mode": "bf16"}
_PREP_JOIN = os.environ.get("VN_PREP_JOIN") == "1"      # A/B aid (read once): the round-2 one-call prepare + full join


def set_precision(mode):
    """'bf16' (bf16 storage + MFMA, BASELINE configs[1]), 'fp32' (exact fp32 MFMA, the parity
    mode), 'fp32x3' (fp32 storage, every conv product as three bf16 MFMAs: ~1e-4 maps, the fast mode inside the 1e-3
    tolerance).  ('bf16x3' was retired in round 5: fp32x3 gives the same map error at four times its speed.)"""
    if mode == "bf16x3":
        raise ValueError("the 'bf16x3' mode was retired (round 5): use 'fp32x3' — same map error, inside the native executor")
    if mode not in E.MODES:
        raise ValueError(mode)
    _PRECISION["mode"] = mode
    E.X3["on"] = mode == "fp32x3"


def get_precision():
    return _PRECISION["mode"]


def _mode():
    return _PRECISION["mode"]


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _lib.VoxelnetHipError("voxelnet_amd modules need CUDA(HIP) tensors; there is no CPU path")


def _need_training(training):
    """(kept for callers; round 3: a backward through an eval-mode forward is supported — the eval-mode BatchNorm backward of
    the reference's autograd (running statistics are constants: dy = S * dz, conv-bias gradient S * d_beta) runs through the
    per-layer orchestration; the native executor handles train-mode steps only and detect() routes accordingly)"""
    return None


def _act_to_nchw(a, dim):
    out = E.rows_to_nchw(Rows(a.t[..., :a.C], a.C), dim)
    if a.lo_off:
        out = out + E.rows_to_nchw(Rows(a.t[..., a.lo_off:a.lo_off + a.C], a.C), dim)
    return out


# ---------------------------------------------------------------------------------------------
# single layers (ConvMD / DeConv2d)
# ---------------------------------------------------------------------------------------------
class _LayerFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, gamma, beta, spec, bn_mod, training):
        _need_cuda(x, weight)
        mode = _mode()
        with _lib.on_device(x.device):
            xr = E.nchw_to_rows(x, mode)
            P = {"weight": weight.detach(), "bias": bias.detach(),
                 "gamma": gamma.detach() if gamma is not None else None,
                 "beta": beta.detach() if beta is not None else None}
            Bf = None
            if spec.bn:
                Bf = {"running_mean": bn_mod.running_mean, "running_var": bn_mod.running_var}
            a, st = E.layer_forward(spec, xr, P, Bf, training, mode, y_dtype=None if spec.bn else torch.float32)
            out = _act_to_nchw(a, spec.dim) if spec.bn else E.rows_to_nchw(a, spec.dim)
        ctx.st, ctx.P, ctx.mode, ctx.spec = st, P, mode, spec
        ctx.need_dx = x.requires_grad
        ctx.training = bool(training) or not spec.bn
        return out

    @staticmethod
    def backward(ctx, dout):
        spec, mode = ctx.spec, ctx.mode
        _need_training(ctx.training)
        with _lib.on_device(dout.device):
            if spec.bn:
                da = E.nchw_to_plain_rows(dout, E.plain_dtype_of(mode))
            else:
                da = E.nchw_to_rows(dout, mode)
            grads, dx = E.layer_backward(ctx.st, da, ctx.P, mode, need_dx=ctx.need_dx)
            dxn = E.rows_to_nchw(dx, spec.dim) if dx is not None else None
        return dxn, grads["weight"], grads["bias"], grads.get("gamma"), grads.get("beta"), None, None, None


def _tup(v, n):
    return tuple(v) if isinstance(v, (tuple, list)) else (v,) * n


class ConvMD(nn.Module):
    """model.py:111-167."""

    def __init__(self, input_dim, cin, cout, kernel_size, stride, padding, bn=True, activation=True):
        super().__init__()
        self.input_dim, self.cin, self.cout = input_dim, cin, cout
        self.kernel_size, self.stride, self.padding = kernel_size, stride, padding
        self.bn, self.activation = bn, activation
        if input_dim == 2:
            self.conv = nn.Conv2d(cin, cout, kernel_size, stride, padding)
            if bn:
                self.batch_norm = nn.BatchNorm2d(cout)
        elif input_dim == 3:
            self.conv = nn.Conv3d(cin, cout, kernel_size, stride, padding)
            if bn:
                self.batch_norm = nn.BatchNorm3d(cout)
        else:
            raise ValueError("Choose between 2D and 3D input.")    # model.py:156
        if bn != activation:
            raise _lib.VoxelnetHipError("ConvMD: only bn==activation variants exist in the reference network")
        k, s, p = _tup(kernel_size, input_dim), _tup(stride, input_dim), _tup(padding, input_dim)
        if input_dim == 2:
            k, s, p = (1,) + k, (1,) + s, (0,) + p
        self._spec = E.LayerSpec("ConvMD", input_dim, cin, cout, k, s, p, bn=bn, relu=activation)

    def forward(self, x):
        bnm = self.batch_norm if self.bn else None
        out = _LayerFn.apply(x, self.conv.weight, self.conv.bias, bnm.weight if bnm is not None else None,
                             bnm.bias if bnm is not None else None, self._spec, bnm, self.training)
        if bnm is not None and self.training:
            bnm.num_batches_tracked += 1
        return out


class DeConv2d(nn.Module):
    """model.py:170-199."""

    def __init__(self, cin, cout, kernel_size, stride, padding, bn=True):
        super().__init__()
        self.cin, self.cout, self.kernel_size, self.stride, self.padding, self.bn = \
            cin, cout, kernel_size, stride, padding, bn
        self.deconv = nn.ConvTranspose2d(cin, cout, kernel_size, stride, padding)
        if bn:
            self.batch_norm = nn.BatchNorm2d(cout)
        else:
            raise _lib.VoxelnetHipError("DeConv2d without BatchNorm does not occur in the reference network")
        k, s, p = _tup(kernel_size, 2), _tup(stride, 2), _tup(padding, 2)
        self._spec = E.LayerSpec("DeConv2d", 2, cin, cout, (1,) + k, (1,) + s, (0,) + p, transposed=True)

    def forward(self, x):
        out = _LayerFn.apply(x, self.deconv.weight, self.deconv.bias, self.batch_norm.weight, self.batch_norm.bias,
                             self._spec, self.batch_norm, self.training)
        if self.training:
            self.batch_norm.num_batches_tracked += 1
        return out


# ---------------------------------------------------------------------------------------------
# feature net (VFE x2 + voxel-wise max + sparse->dense)
# ---------------------------------------------------------------------------------------------
class _VFELayerFn(torch.autograd.Function):
    """VFELayer.forward (model.py:74-82) as one layer through vn_vfe_layer_fwd / vn_vfe_layer_bwd (csrc/vfe_layer.hip)."""

    @staticmethod
    def forward(ctx, inputs, mask, weight, bias, gamma, beta, bn_mod, training):
        _need_cuda(inputs, mask, weight)
        if inputs.dim() != 3 or mask.shape[:2] != inputs.shape[:2]:
            raise ValueError(f"VFELayer: inputs {tuple(inputs.shape)} / mask {tuple(mask.shape)} do not belong together")
        K, T, cin = inputs.shape
        units = weight.shape[0]
        x = inputs.detach().contiguous().float()
        mk = mask.detach().reshape(K, T).ne(0).to(torch.uint8).contiguous()
        w = weight.detach().contiguous()
        with _lib.on_device(x.device):
            ws_bytes = _lib.load().vn_vfe_layer_workspace_bytes(K, T, cin, units)
            if ws_bytes == 0:
                raise _lib.VoxelnetHipError(f"VFELayer({cin}, {2 * units}): cin and cout/2 must be <= 64 on the HIP path")
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
            out = torch.empty((K, T, 2 * units), dtype=torch.float32, device=x.device)
            _lib.call("vn_vfe_layer_fwd", x.data_ptr(), mk.data_ptr(), K, T, cin, units, w.data_ptr(), bias.data_ptr(),
                      gamma.data_ptr(), beta.data_ptr(), bn_mod.running_mean.data_ptr(), bn_mod.running_var.data_ptr(),
                      int(training), E.BN_MOMENTUM, E.BN_EPS, out.data_ptr(), ws.data_ptr(), ws_bytes, E.stream())
        ctx.saved = (x, mk, w, ws, ws_bytes, int(training))
        ctx.need_dx = inputs.requires_grad
        return out

    @staticmethod
    def backward(ctx, d_out):
        x, mk, w, ws, ws_bytes, training = ctx.saved
        K, T, cin = x.shape
        units = w.shape[0]
        d_out = d_out.contiguous().float()
        with _lib.on_device(x.device):
            dx = torch.empty_like(x) if ctx.need_dx else None
            dw = torch.empty_like(w)
            db, dg, dbe = (torch.empty(units, dtype=torch.float32, device=x.device) for _ in range(3))
            _lib.call("vn_vfe_layer_bwd", x.data_ptr(), mk.data_ptr(), d_out.data_ptr(), K, T, cin, units, w.data_ptr(), training,
                      dx.data_ptr() if dx is not None else None, dw.data_ptr(), db.data_ptr(), dg.data_ptr(), dbe.data_ptr(),
                      ws.data_ptr(), ws_bytes, E.stream())
        return dx, None, dw, db, dg, dbe, None, None


def _parts_to(parts, device):
    """[t.to(device) for t in parts] (model.py:302-303) — but a voxelize.VoxelBatch whose tensors already live there is
    returned as it is, with the concatenation it carries"""
    dev = torch.device(device)
    if getattr(parts, "cat", None) is not None and all(t.device == dev for t in parts):
        return parts
    return [t.to(device) for t in parts]


def _batch_cat(parts, dtype):
    """the per-sample tensors of a batch as one (sum K_i, ...) tensor; a voxelize.VoxelBatch brings the concatenation
    along (made on the input pipeline's stream one step ahead), a plain list / tuple is concatenated here"""
    take = getattr(parts, "take", None)
    ready = take() if take is not None else None
    if ready is not None and ready.dtype == dtype:
        return ready
    t = parts[0] if len(parts) == 1 else torch.cat(list(parts), dim=0)
    return t.contiguous().to(dtype)


class VFELayer(nn.Module):
    """model.py:60-82.  Holds fcn (Linear+ReLU) and bn exactly like the reference.  Inside FeatureLearningNet both
    layers and the voxel max run fused (csrc/vfe.hip); called on its own — forward(inputs (K,T,cin), mask (K,T,1)) ->
    (K,T,cout) — the layer runs through its stand-alone kernels (csrc/vfe_layer.hip), forward and backward."""

    def __init__(self, cin, cout):
        super().__init__()
        self.in_channels, self.out_channels, self.local_agg_features = cin, cout, cout // 2
        self.fcn = nn.Sequential(nn.Linear(cin, cout // 2), nn.ReLU())
        self.bn = nn.BatchNorm1d(cout // 2)

    def forward(self, inputs, mask):
        out = _VFELayerFn.apply(inputs, mask, self.fcn[0].weight, self.fcn[0].bias, self.bn.weight, self.bn.bias, self.bn,
                                self.training)
        if self.training:
            self.bn.num_batches_tracked += 1
        return out


VFE_KEYS = ["feature_net.vfe_1.fcn.0.weight", "feature_net.vfe_1.fcn.0.bias", "feature_net.vfe_1.bn.weight",
            "feature_net.vfe_1.bn.bias", "feature_net.vfe_2.fcn.0.weight", "feature_net.vfe_2.fcn.0.bias",
            "feature_net.vfe_2.bn.weight", "feature_net.vfe_2.bn.bias"]


def _vfe_weights(fn):
    v1, v2 = fn.vfe_1, fn.vfe_2
    return [v1.fcn[0].weight, v1.fcn[0].bias, v1.bn.weight, v1.bn.bias,
            v2.fcn[0].weight, v2.fcn[0].bias, v2.bn.weight, v2.bn.bias]


def featnet_forward(feature, params, bufs, training):
    """feature (K,T,7) f32 cuda; params = [w1,b1,g1,be1,w2,b2,g2,be2]; bufs = [rm1,rv1,rm2,rv2].
    -> voxelwise (K,128) f32, stats, saved handle."""
    K, T = feature.shape[0], feature.shape[1]
    dev = feature.device
    w = _lib.VnVfeWeights(params[0].data_ptr(), params[1].data_ptr(), params[2].data_ptr(), params[3].data_ptr(),
                          bufs[0].data_ptr(), bufs[1].data_ptr(), params[4].data_ptr(), params[5].data_ptr(),
                          params[6].data_ptr(), params[7].data_ptr(), bufs[2].data_ptr(), bufs[3].data_ptr())
    ws_bytes = _lib.load().vn_vfe_workspace_bytes(K, T)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    vw = torch.empty((K, 128), dtype=torch.float32, device=dev)
    stats = torch.empty(320, dtype=torch.float32, device=dev)
    with E.section("vfe_fwd", 28.0 * K * T + 512.0 * K):          # (K,T,7) read, (K,128) written
        _lib.call("vn_vfe_fwd", feature.data_ptr(), K, T, ctypes.byref(w), int(training), E.BN_MOMENTUM, E.BN_EPS,
                  vw.data_ptr(), stats.data_ptr(), ws.data_ptr(), ws_bytes, E.stream())
    return vw, stats, (w, ws, ws_bytes)


def featnet_backward(feature, wstruct, stats, d_vw, params, out=None, training=True):
    w, ws, ws_bytes = wstruct
    K, T = feature.shape[0], feature.shape[1]
    grads = out if out is not None else [torch.empty_like(p) for p in params]
    g = _lib.VnVfeGrads(*[t.data_ptr() for t in grads])
    d_vw = d_vw.contiguous()
    # (ws is the forward's workspace, kept alive and untouched by the saved handle: its work list is reused)
    with E.section("vfe_bwd", 2.0 * (28.0 * K * T + 512.0 * K)):
        _lib.call("vn_vfe_bwd", feature.data_ptr(), K, T, ctypes.byref(w), stats.data_ptr(), d_vw.data_ptr(),
                  ctypes.byref(g), ws.data_ptr(), ws_bytes, 1 | (0 if training else 2), E.stream())
    return grads


def scatter_rows(vw, coord, B, dims, mode):
    """model.py:102-106 -> dense Rows in the mode's activation format"""
    D, H, W = dims
    K, C = vw.shape
    split = E.is_split(mode)
    ch = 2 * C if split else C
    dense = torch.empty((B, D, H, W, ch), dtype=E.act_dtype_of(mode), device=vw.device)
    _lib.call("vn_scatter_dense_fwd", vw.data_ptr(), coord.data_ptr(), K, C, B, D, H, W, dense.data_ptr(),
              E._dt(dense), ch, int(split), E.stream())
    return Rows(dense, C, C if split else 0)


def gather_rows(d_dense, coord, K, C):
    """backward of the scatter: rows of d_dense (plain f32/bf16 Rows) at coord -> (K,C) f32"""
    B = d_dense.B
    D, H, W = d_dense.dims
    out = torch.empty((K, C), dtype=torch.float32, device=coord.device)
    _lib.call("vn_scatter_dense_bwd", d_dense.ptr(), E._dt(d_dense.t), coord.data_ptr(), K, C, B, D, H, W,
              out.data_ptr(), E.stream())
    return out


class _FeatureNetFn(torch.autograd.Function):
    """FeatureLearningNet.forward with the fp32 dense output of the reference (module boundary)."""

    @staticmethod
    def forward(ctx, feature, coord, B, dims, training, bufs, *params):
        _need_cuda(feature, coord)
        params = [p.detach() for p in params]
        with _lib.on_device(feature.device):
            vw, stats, wst = featnet_forward(feature, params, bufs, training)
            D, H, W = dims
            dense = torch.empty((B, D, H, W, 128), dtype=torch.float32, device=feature.device)
            _lib.call("vn_scatter_dense_fwd", vw.data_ptr(), coord.data_ptr(), vw.shape[0], 128, B, D, H, W,
                      dense.data_ptr(), _lib.VN_F32, 128, 0, E.stream())
        ctx.saved = (feature, coord, stats, wst, params)
        ctx.training = bool(training)
        return dense

    @staticmethod
    def backward(ctx, d_dense):
        _need_training(ctx.training)
        feature, coord, stats, wst, params = ctx.saved
        with _lib.on_device(d_dense.device):
            d_vw = gather_rows(Rows(d_dense.contiguous(), 128), coord, feature.shape[0], 128)
            grads = featnet_backward(feature, wst, stats, d_vw, params, training=ctx.training)
        return (None, None, None, None, None, None) + tuple(grads)


class FeatureLearningNet(nn.Module):
    """model.py:85-108.  forward(feature: list[(K_i,T,7)], coordinate: list[(K_i,4)]) -> (B,D,H,W,128)."""

    def __init__(self, cls_name="Car"):
        super().__init__()
        self.vfe_1 = VFELayer(7, 32)
        self.vfe_2 = VFELayer(32, 128)
        self._grid = grid_config(cls_name)

    def _bufs(self):
        return [self.vfe_1.bn.running_mean, self.vfe_1.bn.running_var, self.vfe_2.bn.running_mean,
                self.vfe_2.bn.running_var]

    def _tick(self):
        if self.training:
            self.vfe_1.bn.num_batches_tracked += 1
            self.vfe_2.bn.num_batches_tracked += 1

    def forward(self, feature, coordinate):
        bs = len(feature)
        feature, coordinate = _batch_cat(feature, torch.float32), _batch_cat(coordinate, torch.int64)
        out = _FeatureNetFn.apply(feature, coordinate, bs, self._grid.dims, self.training, self._bufs(),
                                  *_vfe_weights(self))
        self._tick()
        return out


# ---------------------------------------------------------------------------------------------
# middle layers + RPN
# ---------------------------------------------------------------------------------------------
def _collect_middle(mod):
    """-> (names, P, Bf, flat parameter list) in net.layer_table order, + heads"""
    names, P, Bf, flat = [], {}, {}, []
    for name, spec in N.layer_table(mod._block1_stride):
        blk, _, idx = name.partition(".")
        m = getattr(mod, blk)
        if idx:
            m = m[int(idx)]
        conv = m.deconv if spec.transposed else m.conv
        bn = m.batch_norm
        P[name] = {"weight": conv.weight, "bias": conv.bias, "gamma": bn.weight, "beta": bn.bias}
        Bf[name] = {"running_mean": bn.running_mean, "running_var": bn.running_var}
        names.append(name)
        flat += [conv.weight, conv.bias, bn.weight, bn.bias]
    flat += [mod.prob_conv.conv.weight, mod.prob_conv.conv.bias, mod.reg_conv.conv.weight, mod.reg_conv.conv.bias]
    return names, P, Bf, flat


def _heads_params(flat):
    pw, pb, rw, rb = flat[-4:]      # (the last four of the flat parameter list: prob / reg weight and bias)
    return {"weight": torch.cat([pw, rw], 0).contiguous(), "bias": torch.cat([pb, rb], 0).contiguous()}


def _middle_grads_flat(names, G):
    out = []
    for n in names:
        g = G[n]
        out += [g["weight"], g["bias"], g["gamma"], g["beta"]]
    hw, hb = G["heads"]["weight"], G["heads"]["bias"]
    out += [hw[:2].contiguous(), hb[:2].contiguous(), hw[2:].contiguous(), hb[2:].contiguous()]
    return out


def _detached(P):
    return {k: {kk: vv.detach() for kk, vv in v.items()} for k, v in P.items()}


def _dir_grads(ctx, G):
    """the direction head's two gradients behind a Function's other outputs: () without the head, (None, None) when its
    logits had no gradient"""
    if not ctx.dir_head:
        return ()
    g = G.get("dir_head")
    return (None, None) if g is None else (g["weight"], g["bias"])


def _dir_params(mid):
    return [mid.dir_conv.conv.weight, mid.dir_conv.conv.bias]


def _iou_params(mid):
    return [mid.iou_conv.conv.weight, mid.iou_conv.conv.bias]


def _iou_grads(ctx, G):
    """_dir_grads for the IoU-aware head, whose two parameters travel behind the direction head's"""
    if not ctx.iou_head:
        return ()
    g = G.get("iou_head")
    return (None, None) if g is None else (g["weight"], g["bias"])


def _peel_site_heads(has_dir, has_iou, flat):
    """flat = (..., [dir weight, bias], [iou weight, bias]) -> (dirp, ioup, the rest): each head's detached pair or None"""
    dirp = ioup = None
    if has_iou:
        ioup, flat = tuple(f.detach() for f in flat[-2:]), flat[:-2]
    if has_dir:
        dirp, flat = tuple(f.detach() for f in flat[-2:]), flat[:-2]
    return dirp, ioup, flat


def _head_out_grads(ctx, d_heads):
    """the gradients of the site heads' logits, which follow (prob, reg) in a Function's outputs -> (d_dir, d_iou)"""
    d = list(d_heads)
    d_dir = d.pop(0) if ctx.dir_head and d else None
    d_iou = d.pop(0) if ctx.iou_head and d else None
    return d_dir, d_iou


class _MiddleFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, mod, training, *flat):
        _need_cuda(x)
        mode = _mode()
        names, P, Bf, _ = _collect_middle(mod)
        P = _detached(P)
        # (the direction head's two parameters travel last, the IoU-aware head's two behind them)
        dirp, ioup, flat = _peel_site_heads(getattr(mod, "dir_conv", None) is not None, getattr(mod, "iou_conv", None) is not None, flat)
        P["heads"] = _heads_params([f.detach() for f in flat])
        with _lib.on_device(x.device):
            B, D, H, W, C = x.shape
            xc = x.contiguous().float()
            if E.is_f32_storage(mode):
                dense = Rows(xc, 128)
            else:
                dense = E.new_rows(B, (D, H, W), 128, torch.bfloat16, E.is_split(mode), x.device)
                _lib.call("vn_cast_rows", xc.data_ptr(), _lib.VN_F32, 128, B * D * H * W, 128, dense.ptr(),
                          _lib.VN_BF16, dense.t.shape[-1], dense.lo_off, E.stream())
            out = N.middle_forward(dense, P, Bf, mod._block1_stride, training, mode, dir_head=dirp, iou_head=ioup)
        st = out[-1]
        ctx.st, ctx.P, ctx.names = st, P, names
        ctx.need_dx = x.requires_grad
        ctx.training = bool(training)
        ctx.dir_head, ctx.iou_head = dirp is not None, ioup is not None
        return out[:-1]

    @staticmethod
    def backward(ctx, d_prob, d_reg, *d_heads):
        _need_training(ctx.training)
        d_dir, d_iou = _head_out_grads(ctx, d_heads)
        with _lib.on_device(d_prob.device):
            G, d_dense = N.middle_backward(ctx.st, d_prob.float(), d_reg.float(), ctx.P, need_dx=ctx.need_dx, d_dir=d_dir, d_iou=d_iou)
            dx = None
            if d_dense is not None:
                dx = d_dense.t if d_dense.t.dtype == torch.float32 else d_dense.t.float()
        return (dx, None, None) + tuple(_middle_grads_flat(ctx.names, G)) + _dir_grads(ctx, G) + _iou_grads(ctx, G)


class MiddleConvNet(nn.Module):
    """model.py:202-281.  forward(x (B,D,H,W,128)) -> (sigmoid(probs) (B,2,h,w), reg (B,14,h,w))."""

    last_dir_logits = None   # the direction head's latest logits (dir_conv is registered by dir_head=True only)

    last_iou_logits = None   # the IoU-aware head's latest logits (iou_conv is registered by iou_head=True only)

    def __init__(self, cls_name="Car", dir_head=False, iou_head=False):
        super().__init__()
        g = grid_config(cls_name)
        self._block1_stride = g.block1_stride
        self.middle_layer = nn.Sequential(
            ConvMD(3, 128, 64, 3, (2, 1, 1), (1, 1, 1)),
            ConvMD(3, 64, 64, 3, (1, 1, 1), (0, 1, 1)),
            ConvMD(3, 64, 64, 3, (2, 1, 1), (1, 1, 1)))
        s1 = (g.block1_stride, g.block1_stride)                    # model.py:212-227
        self.block1 = nn.Sequential(ConvMD(2, 128, 128, 3, s1, (1, 1)),
                                    *[ConvMD(2, 128, 128, 3, (1, 1), (1, 1)) for _ in range(4)])
        self.deconv1 = DeConv2d(128, 256, 3, (1, 1), (1, 1))
        self.block2 = nn.Sequential(ConvMD(2, 128, 128, 3, (2, 2), (1, 1)),
                                    *[ConvMD(2, 128, 128, 3, (1, 1), (1, 1)) for _ in range(5)])
        self.deconv2 = DeConv2d(128, 256, 2, (2, 2), (0, 0))
        self.block3 = nn.Sequential(ConvMD(2, 128, 256, 3, (2, 2), (1, 1)),
                                    *[ConvMD(2, 256, 256, 3, (1, 1), (1, 1)) for _ in range(5)])
        self.deconv3 = DeConv2d(256, 256, 4, (4, 4), (0, 0))
        self.prob_conv = ConvMD(2, 768, 2, 1, (1, 1), (0, 0), bn=False, activation=False)
        self.reg_conv = ConvMD(2, 768, 14, 1, (1, 1), (0, 0), bn=False, activation=False)
        if dir_head:
            self.dir_conv = ConvMD(2, 768, 2, 1, (1, 1), (0, 0), bn=False, activation=False)
        if iou_head:
            self.iou_conv = ConvMD(2, 768, 2, 1, (1, 1), (0, 0), bn=False, activation=False)
            nn.init.zeros_(self.iou_conv.conv.bias)          # (q starts around 1/2 whatever the features' offset)
        # config.py FEATURE_HEIGHT/WIDTH: car 200x176; ped/cyc 100x120 (although the network emits 200x240,
        # SURVEY.md §8a a8 — kept as the reference has it)
        self.output_shape = [g.H // 2, g.W // 2]

    def __getstate__(self):               # (see RPN3D.__getstate__: runtime caches do not travel with a pickle / deepcopy)
        d = self.__dict__.copy()
        d.pop("_native_arrays", None)
        d.pop("_nbt", None)
        d.pop("last_dir_logits", None)
        d.pop("last_iou_logits", None)
        return d

    def _tick(self):
        if self.training:
            ctrs = self.__dict__.get("_nbt")
            if ctrs is None or ctrs[0].device != self.prob_conv.conv.weight.device:
                ctrs = [m.num_batches_tracked for m in self.modules() if isinstance(m, (nn.BatchNorm2d, nn.BatchNorm3d))]
                self.__dict__["_nbt"] = ctrs
            torch._foreach_add_(ctrs, 1)

    def forward(self, x):
        _, _, _, flat = _collect_middle(self)
        has_dir, has_iou = getattr(self, "dir_conv", None) is not None, getattr(self, "iou_conv", None) is not None
        if has_dir or has_iou:       # (same two outputs; the heads' logits are kept as last_dir_logits / last_iou_logits)
            if E.X3["on"]:
                raise ValueError(f"{'dir_head' if has_dir else 'iou_head'}: the fp32x3 mode is not supported with the "
                                 f"{'direction' if has_dir else 'IoU-aware'} head (DESIGN.md {'1i' if has_dir else '1l'})")
            extra = (_dir_params(self) if has_dir else []) + (_iou_params(self) if has_iou else [])
            out = list(_MiddleFn.apply(x, self, self.training, *flat, *extra))
            prob, reg = out[0], out[1]
            if has_dir:
                self.last_dir_logits = out[2]
            if has_iou:
                self.last_iou_logits = out[-1]
        else:
            prob, reg = _MiddleFn.apply(x, self, self.training, *flat)
        self._tick()
        return prob, reg


_BWD_ORDER = [22] + list(range(21, 15, -1)) + [15] + list(range(14, 8, -1)) + [8] + list(range(7, 2, -1)) + [2, 1, 0]

# backward segments of the native executor (vn_net_backward steps) that complete a DDP bucket each
# (parallel.BUCKET_PLAN): heads+deconv3+block3 | deconv2+block2+deconv1 | block1 | middle_layer (the VFE bucket follows)
NATIVE_SEGMENTS = [(0, 8), (8, 16), (16, 21), (21, 24)]


def _native_layer_arrays(mid, grad_views=None):
    """ctypes arrays of vnLayerParams (and vnLayerGrads) in execution order.  Cached on the module: building them walks
    23 layers x 10 attributes (~0.2 ms of host time per call, twice per step); the key is the data pointer of the first
    and last parameter / running buffer / gradient view, which change whenever the storage behind them does
    (`.to()`, a new flat gradient buffer, a reducer's buckets)."""
    table = N.layer_table(mid._block1_stride)
    first, last = getattr(mid, table[0][0].partition(".")[0])[0], mid.deconv3
    key = (first.conv.weight.data_ptr(), first.batch_norm.running_mean.data_ptr(), last.deconv.weight.data_ptr(),
           last.batch_norm.running_var.data_ptr(), mid._block1_stride)
    if grad_views is not None:
        key += (grad_views["middle_rpn.middle_layer.0.conv.weight"].data_ptr(),
                grad_views["middle_rpn.deconv3.batch_norm.bias"].data_ptr())
    cache = mid.__dict__.setdefault("_native_arrays", {})
    hit = cache.get(grad_views is not None)
    if hit is not None and hit[0] == key:
        return hit[1], hit[2]
    arr = (_lib.VnLayerParams * len(table))()
    garr = (_lib.VnLayerGrads * len(table))() if grad_views is not None else None
    for i, (name, spec) in enumerate(table):
        blk, _, idx = name.partition(".")
        m = getattr(mid, blk)
        if idx:
            m = m[int(idx)]
        conv = m.deconv if spec.transposed else m.conv
        bn = m.batch_norm
        arr[i] = _lib.VnLayerParams(conv.weight.data_ptr(), conv.bias.data_ptr(), bn.weight.data_ptr(),
                                    bn.bias.data_ptr(), bn.running_mean.data_ptr(), bn.running_var.data_ptr())
        if garr is not None:
            cv = "deconv" if spec.transposed else "conv"
            pre = f"middle_rpn.{name}."
            garr[i] = _lib.VnLayerGrads(grad_views[pre + cv + ".weight"].data_ptr(), grad_views[pre + cv + ".bias"].data_ptr(),
                                        grad_views[pre + "batch_norm.weight"].data_ptr(),
                                        grad_views[pre + "batch_norm.bias"].data_ptr())
    cache[grad_views is not None] = (key, arr, garr)
    return arr, garr


HEADS_W, HEADS_B = "__heads_weight_fused__", "__heads_bias_fused__"


def _grad_views(rpn, fresh=False):
    """name -> gradient tensor the kernels write into: the DDP buckets' views when a reducer is attached, else
    views of one persistent flat buffer owned by the module (no per-step allocation of 104 tensors).
    fresh=True: a new, uncached buffer (gradient accumulation: the persistent one may BE the parameters' .grad)."""
    if rpn.grad_reducer is not None and not fresh:
        hit = rpn.__dict__.get("_bucket_views")
        if hit is None or hit[0] is not rpn.grad_reducer:
            out = {}
            for b in rpn.grad_reducer.buckets:
                out.update(b["views"])
            out.update(getattr(rpn.grad_reducer, "fused_views", {}))
            hit = (rpn.grad_reducer, out)
            rpn.__dict__["_bucket_views"] = hit
        return hit[1]
    named = rpn._named_params()
    key = tuple((n, p.data_ptr()) for n, p in named[:2]) + (named[0][1].device,)
    cache = None if fresh else rpn.__dict__.get("_flat_grads")
    if cache is None or cache[0] != key:
        total = sum(p.numel() for _, p in named)
        flat = torch.zeros(total, dtype=torch.float32, device=named[0][1].device)
        # the two heads' weights (and biases) are laid out back to back, so that the executor's fused (16,768) heads
        # gradient IS the two parameters' gradients: no split copies (HEADS_W / HEADS_B name the fused views)
        hw = ["middle_rpn.prob_conv.conv.weight", "middle_rpn.reg_conv.conv.weight"]
        hb = ["middle_rpn.prob_conv.conv.bias", "middle_rpn.reg_conv.conv.bias"]
        byname = dict(named)
        order = [n for n, _ in named if n not in hw + hb] + hw + hb
        views, off, start = {}, 0, {}
        for n in order:
            p_ = byname[n]
            start[n] = off
            views[n] = flat[off:off + p_.numel()].view_as(p_)
            off += p_.numel()
        views[HEADS_W] = flat[start[hw[0]]:start[hw[0]] + 16 * 768].view(16, 768, 1, 1)
        views[HEADS_B] = flat[start[hb[0]]:start[hb[0]] + 16]
        cache = (key, flat, views)
        if not fresh:
            rpn.__dict__["_flat_grads"] = cache
    return cache[2]


class _DetectorFn(torch.autograd.Function):
    """feature_net + middle_rpn fused: the dense grid is written once, directly in the conv
    kernels' bf16 / [hi|lo] row format, and never exists as an fp32 NDHWC tensor."""

    @staticmethod
    def forward(ctx, feature, coord, B, rpn, training, *flat):
        _need_cuda(feature, coord)
        mode = _mode()
        fn, mid = rpn.feature_net, rpn.middle_rpn
        nv = 8
        # anchor mode (RPN3D.detect): the 104 parameters do not travel through autograd — a single one-element tensor that
        # requires grad stands for them, and the backward assigns / adds the gradients to .grad itself (what the direct_grads
        # mode did anyway): wrapping and unwrapping 104 inputs and their AccumulateGrad edges cost ~0.4 ms of host time a step
        ctx.anchor = len(flat) == 1
        dirp = ioup = None
        if not ctx.anchor:       # (the direction head's two parameters travel last, the IoU-aware head's behind them)
            dirp, ioup, flat = _peel_site_heads(bool(rpn.dir_head), bool(rpn.iou_head), flat)
        ctx.dir_head, ctx.iou_head = dirp is not None, ioup is not None
        if ctx.anchor:
            flat = rpn._flat_params()
            vparams = flat[:nv]
        else:
            vparams = [p.detach() for p in flat[:nv]]
        # the native executor's backward is the train-mode one: an eval-mode forward that will be differentiated goes through
        # the per-layer orchestration (eval-mode BatchNorm backward, engine.layer_backward)
        native = rpn._native_ok(mode) and (bool(training) or not any(ctx.needs_input_grad))   # (all False under no_grad: detect)
        if ctx.anchor and not native:
            raise _lib.VoxelnetHipError("internal: the one-tensor (anchor) call needs the native executor (RPN3D._native_ok)")
        if not native:          # (the per-launch Python orchestration works on name -> tensor dicts)
            names, P, Bf, _ = _collect_middle(mid)
            P = _detached(P)
            P["heads"] = _heads_params([f.detach() for f in flat[-4:]])
        if native:
            with _lib.on_device(feature.device):
                dev_ = feature.device
                sparse = bool(rpn.sparse_first_layer)
                D, H, W = fn._grid.dims
                K = feature.shape[0]
                cfg = _lib.VnNetConfig(B, D, H, W, mid._block1_stride, {"bf16": 0, "fp32": 1, "fp32x3": 2}[mode], int(training), int(sparse), 0, 0)
                cfg.grad_storage = int(rpn.grad_storage) & (16 if E.is_f32_storage(mode) else 15)
                side = rpn._side_stream(dev_) if rpn.overlap_wgrad else None
                arr, _ = _native_layer_arrays(mid)
                lib = _lib.load()
                ws_bytes = lib.vn_net_workspace_bytes(ctypes.byref(cfg), K)
                if ws_bytes == 0:
                    raise _lib.VoxelnetHipError("vn_net_workspace_bytes: unsupported network configuration")
                ws = rpn._ws_acquire(ws_bytes, dev_)
                if side is not None:
                    # what does not depend on the voxel features runs on the side stream beside the VFE forward, the first
                    # layer's needs first (its packed weights, the site list, the index grid: vn_net_prepare's two-call
                    # form), then the (16,768) / (16,) concatenations of the two heads' parameters — two small launches the
                    # weight packing reads — and the rest of the packing
                    side_t = rpn.__dict__["_side"]
                    side_t.wait_stream(_lib.current_stream(dev_))
                    two_phase = not _PREP_JOIN      # ("1": the round-2 schedule, one call, for A/B runs)
                    if two_phase:
                        cfg.prepared = 1                       # phase 1: the first layer's needs only
                        _lib.call("vn_net_prepare", rpn._net_handle(dev_), ctypes.byref(cfg), arr, None, coord.data_ptr(), K,
                                  ws.data_ptr(), ws_bytes, side)
                    with torch.cuda.stream(side_t):
                        heads = _heads_params([f.detach() for f in flat[-4:]])
                    for t_ in heads.values():
                        t_.record_stream(_lib.current_stream(dev_))
                    cfg.prepared = 2 if two_phase else 0       # phase 2: the rest (0: everything in this one call)
                    _lib.call("vn_net_prepare", rpn._net_handle(dev_), ctypes.byref(cfg), arr, heads["weight"].data_ptr(), coord.data_ptr(), K,
                              ws.data_ptr(), ws_bytes, side)
                    cfg.prepared = 1
                else:
                    heads = _heads_params([f.detach() for f in flat[-4:]])
                vw, stats, wst = featnet_forward(feature, vparams, fn._bufs(), training)
                # With the sparse first Conv3d (rulebook evaluation: voxel rows x packed weights, then a gather-sum per
                # active site) the dense (B,10,400,352,128) grid of model.py:102-106 is never built.
                dense = None if sparse else scatter_rows(vw, coord, B, fn._grid.dims, mode)
                if E.is_f32_storage(mode):
                    vw_rows = vw.bfloat16().float() if cfg.grad_storage & 16 else vw      # (diagnostic: see vnNetConfig)
                else:
                    vw_rows = torch.empty((vw.shape[0], 128), dtype=torch.bfloat16, device=vw.device)
                    _lib.call("vn_cast_rows", vw.data_ptr(), _lib.VN_F32, 128, vw.shape[0], 128, vw_rows.data_ptr(),
                              _lib.VN_BF16, 128, 0, E.stream())
                # (no join of the side stream here: vn_net_forward waits for vn_net_prepare's two events itself — the first
                # layer's needs at its start, the rest of the weight packing in front of the second layer)
                if side is not None and _PREP_JOIN:     # A/B aid: the round-2 full join
                    torch.cuda.current_stream().wait_stream(side_t)
                hf, wf = H // mid._block1_stride, W // mid._block1_stride
                prob = torch.empty((B, 2, hf, wf), dtype=torch.float32, device=vw.device)
                reg = torch.empty((B, 14, hf, wf), dtype=torch.float32, device=vw.device)
                _lib.call("vn_net_forward", rpn._net_handle(dev_), ctypes.byref(cfg), arr, heads["weight"].data_ptr(), heads["bias"].data_ptr(),
                          dense.ptr() if dense is not None else None, coord.data_ptr(), vw_rows.data_ptr(), K, ws.data_ptr(),
                          ws_bytes, prob.data_ptr(), reg.data_ptr(), E.stream(), side)
            ctx.saved = (feature, coord, stats, wst, vparams, (cfg, ws, ws_bytes, dense, vw_rows, heads, prob.detach()), None, None)
            # (prob.detach(): an alias — keeping the Function's own output on ctx would be a reference cycle)
            ctx.reducer = rpn.grad_reducer
            ctx.rpn = rpn
            ctx.native = True
            ctx.training = bool(training)
            if not any(ctx.needs_input_grad):      # forward-only call: nothing will read the arena again
                rpn._ws_release(ws)
            return prob, reg
        ctx.native = False
        with _lib.on_device(feature.device):
            vw, stats, wst = featnet_forward(feature, vparams, fn._bufs(), training)
            dense = scatter_rows(vw, coord, B, fn._grid.dims, mode)
            sparse = None
            if rpn.sparse_first_layer and not E.is_split(mode):
                if E.is_f32_storage(mode):
                    vw_rows = vw
                else:
                    vw_rows = torch.empty((vw.shape[0], 128), dtype=torch.bfloat16, device=vw.device)
                    _lib.call("vn_cast_rows", vw.data_ptr(), _lib.VN_F32, 128, vw.shape[0], 128, vw_rows.data_ptr(),
                              _lib.VN_BF16, 128, 0, E.stream())
                sparse = (coord, vw_rows)
            out = N.middle_forward(dense, P, Bf, mid._block1_stride, training, mode, sparse=sparse, dir_head=dirp, iou_head=ioup)
        st = out[-1]
        ctx.saved = (feature, coord, stats, wst, vparams, st, P, names)
        ctx.reducer = rpn.grad_reducer
        ctx.training = bool(training)
        return out[:-1]

    @staticmethod
    def backward(ctx, d_prob, d_reg, *d_heads):
        _need_training(ctx.training)
        d_dir, d_iou = _head_out_grads(ctx, d_heads)
        feature, coord, stats, wst, vparams, st, P, names = ctx.saved
        red = ctx.reducer
        if ctx.native:
            return _DetectorFn._backward_native(ctx, d_prob, d_reg)
        on_grads = None
        if red is not None:
            def on_grads(name, g):
                if name == "heads":
                    hw, hb = g["weight"], g["bias"]
                    red.grad_ready("middle_rpn.prob_conv.conv.weight", hw[:2])
                    red.grad_ready("middle_rpn.prob_conv.conv.bias", hb[:2])
                    red.grad_ready("middle_rpn.reg_conv.conv.weight", hw[2:])
                    red.grad_ready("middle_rpn.reg_conv.conv.bias", hb[2:])
                    return
                cv = "deconv" if name.startswith("deconv") else "conv"
                red.grad_ready(f"middle_rpn.{name}.{cv}.weight", g["weight"])
                red.grad_ready(f"middle_rpn.{name}.{cv}.bias", g["bias"])
                red.grad_ready(f"middle_rpn.{name}.batch_norm.weight", g["gamma"])
                red.grad_ready(f"middle_rpn.{name}.batch_norm.bias", g["beta"])
        with _lib.on_device(d_prob.device):
            G, d_dense = N.middle_backward(st, d_prob.float(), d_reg.float(), P, need_dx=True, on_grads=on_grads, d_dir=d_dir, d_iou=d_iou)
            d_vw = d_dense if torch.is_tensor(d_dense) else gather_rows(d_dense, coord, feature.shape[0], 128)
            vg = featnet_backward(feature, wst, stats, d_vw, vparams, training=ctx.training)
            if red is not None:
                for key, g in zip(VFE_KEYS, vg):
                    red.grad_ready(key, g)
        return (None, None, None, None, None) + tuple(vg) + tuple(_middle_grads_flat(names, G)) + _dir_grads(ctx, G) + _iou_grads(ctx, G)


def _detector_backward_segments(cfg, arr, heads, dp, dr, prob, dense, coord, vw_rows, K, ws, ws_bytes, garr, dhw, dhb, d_in,
                                side, red, views, table, order, rpn, feature, wst, stats, d_vw, vparams):
    """the executor's backward as one call (no reducer) or one call per DDP bucket (reducer without a comm stream)"""
    mid = rpn.middle_rpn
    if True:
        # one segment per DDP bucket when gradients are all-reduced while the backward runs; else a single call
        # (fewer fork/join points for the side stream, one unpack launch)
        segments = NATIVE_SEGMENTS if red is not None else [(0, 24)]
        # without a reducer the last weight gradients (side stream) may still run while the VFE backward goes on:
        # the executor leaves the join to us (cfg.defer_join), we wait for the side stream after featnet_backward
        cfg.defer_join = int(side is not None and red is None)
        for sb, se in segments:
            _lib.call("vn_net_backward", rpn._net_handle(dp.device), ctypes.byref(cfg), arr, heads["weight"].data_ptr(), dp.data_ptr(), dr.data_ptr(),
                      prob.data_ptr(), dense.ptr() if dense is not None else None, coord.data_ptr(), vw_rows.data_ptr(), K,
                      ws.data_ptr(), ws_bytes, garr,
                      dhw.data_ptr(), dhb.data_ptr(), d_in.data_ptr(), sb, se, E.stream(), side)
            if sb == 0 and not cfg.defer_join:
                _split_heads_grads(views, dhw, dhb)
            if red is not None:
                names = []
                if sb == 0:
                    names += ["middle_rpn.prob_conv.conv.weight", "middle_rpn.prob_conv.conv.bias",
                              "middle_rpn.reg_conv.conv.weight", "middle_rpn.reg_conv.conv.bias"]
                for step in range(max(sb, 1), se):
                    name, spec = table[order[step - 1]]
                    cv = "deconv" if spec.transposed else "conv"
                    names += [f"middle_rpn.{name}.{cv}.weight", f"middle_rpn.{name}.{cv}.bias",
                              f"middle_rpn.{name}.batch_norm.weight", f"middle_rpn.{name}.batch_norm.bias"]
                for n in names:       # (with a reducer the call has joined the side stream: the group's gradients are final —
                    red.grad_ready(n, views[n])      # the middle_layer bucket too, which then runs beside the VFE backward)
        if not cfg.sparse_first:
            d_vw = gather_rows(Rows(d_in, 128), coord, K, 128)
        vg = featnet_backward(feature, wst, stats, d_vw, vparams, out=[views[k] for k in VFE_KEYS])
        if cfg.defer_join:
            torch.cuda.current_stream().wait_stream(rpn.__dict__["_side"])
            _split_heads_grads(views, dhw, dhb)      # (dhw is written by the unpack, which ran on the side stream)
        if red is not None:
            for n in VFE_KEYS:
                red.grad_ready(n, views[n])
    return vg


def _split_heads_grads(views, dhw, dhb):
    """fused (16,768) heads gradient -> prob_conv / reg_conv parameter gradients (model.py:276-279); nothing to do when
    the gradient views are laid out as that fused block (_grad_views)"""
    if HEADS_W in views:
        return
    views["middle_rpn.prob_conv.conv.weight"].copy_(dhw[:2])
    views["middle_rpn.prob_conv.conv.bias"].copy_(dhb[:2])
    views["middle_rpn.reg_conv.conv.weight"].copy_(dhw[2:])
    views["middle_rpn.reg_conv.conv.bias"].copy_(dhb[2:])


def _detector_backward_native(ctx, d_prob, d_reg):
    feature, coord, stats, wst, vparams, nat, _, _ = ctx.saved
    cfg, ws, ws_bytes, dense, vw_rows, heads, prob = nat
    rpn, red = ctx.rpn, ctx.reducer
    mid = rpn.middle_rpn
    K = feature.shape[0]
    dev = d_prob.device
    # Some parameter already has a .grad (a second backward() before zero_grad, or zero_grad(set_to_none=False)): the
    # caller wants SUMS.  The persistent flat buffer may BE those .grad tensors (direct_grads), so the kernels must not
    # overwrite it: this step's gradients go to a fresh buffer and are handed to autograd, whose AccumulateGrad adds.
    plist = rpn._flat_params()
    accumulate = any(p.grad is not None for p in plist)
    if accumulate and red is not None:
        raise _lib.VoxelnetHipError("gradient accumulation over several backward() calls is not supported with a "
                                    "grad_reducer attached: call zero_grad(set_to_none=True) after every step")
    views = _grad_views(rpn, fresh=accumulate)
    with _lib.on_device(dev):
        arr, garr = _native_layer_arrays(mid, views)
        fused_heads = HEADS_W in views          # flat buffer: the fused heads gradient is written in place
        dhw = views[HEADS_W] if fused_heads else torch.empty((16, 768, 1, 1), dtype=torch.float32, device=dev)
        dhb = views[HEADS_B] if fused_heads else torch.empty(16, dtype=torch.float32, device=dev)
        d_vw = torch.empty((K, 128), dtype=torch.float32, device=dev)
        dp, dr = d_prob.contiguous().float(), d_reg.contiguous().float()
        d_in = d_vw if cfg.sparse_first else torch.empty_like(dense.t)
        table = N.layer_table(mid._block1_stride)
        order = _BWD_ORDER
        side = rpn._side_stream(dev) if rpn.overlap_wgrad else None
        if red is not None and side is not None and red.comm_stream is not None:
            # Gradient all-reduce overlapped with a SINGLE backward call: the executor unpacks every parameter group's
            # weight gradients on the side stream and records "group final" events; the comm stream waits for them
            # (vn_net_wait_bucket) — the compute streams never stall for the reducer.
            cfg.bucket_events, cfg.defer_join = 1, 1
            _lib.call("vn_net_backward", rpn._net_handle(dev), ctypes.byref(cfg), arr, heads["weight"].data_ptr(), dp.data_ptr(), dr.data_ptr(),
                      prob.data_ptr(), dense.ptr() if dense is not None else None, coord.data_ptr(), vw_rows.data_ptr(), K,
                      ws.data_ptr(), ws_bytes, garr, dhw.data_ptr(), dhb.data_ptr(), d_in.data_ptr(), 0, 24, E.stream(), side)

            def waiter(bi):
                return lambda st: _lib.call("vn_net_wait_bucket", rpn._net_handle(dev), bi, ctypes.c_void_p(st.cuda_stream))
            dhw.record_stream(red.comm_stream)       # read there (prelude) after this function has returned
            dhb.record_stream(red.comm_stream)
            red.launch_bucket(0, wait_fn=waiter(0), prelude=lambda: _split_heads_grads(views, dhw, dhb))
            red.launch_bucket(1, wait_fn=waiter(1))
            red.launch_bucket(2, wait_fn=waiter(2))
            red.launch_bucket(3, wait_fn=waiter(3))          # middle_layer: runs beside the VFE backward
            if not cfg.sparse_first:
                d_vw = gather_rows(Rows(d_in, 128), coord, K, 128)
            vg = featnet_backward(feature, wst, stats, d_vw, vparams, out=[views[k] for k in VFE_KEYS])
            vfe_done = torch.cuda.Event()
            vfe_done.record()
            red.launch_bucket(4, after_event=vfe_done)      # the 9.6 KB of VFE gradients: the exposed tail
            torch.cuda.current_stream().wait_stream(rpn.__dict__["_side"])
        else:
            # one segment per DDP bucket when gradients are all-reduced while the backward runs (no side stream); else
            # a single call (fewer fork/join points for the side stream, one unpack launch)
            vg = _detector_backward_segments(cfg, arr, heads, dp, dr, prob, dense, coord, vw_rows, K, ws, ws_bytes, garr,
                                             dhw, dhb, d_in, side, red, views, table, order, rpn, feature, wst, stats, d_vw,
                                             vparams)
    hit = None if accumulate else rpn.__dict__.get("_mg_cache")
    if hit is None or hit[0] is not views:
        mg = []
        for name, spec in table:
            cv = "deconv" if spec.transposed else "conv"
            pre = f"middle_rpn.{name}."
            mg += [views[pre + cv + ".weight"], views[pre + cv + ".bias"], views[pre + "batch_norm.weight"],
                   views[pre + "batch_norm.bias"]]
        mg += [views["middle_rpn.prob_conv.conv.weight"], views["middle_rpn.prob_conv.conv.bias"],
               views["middle_rpn.reg_conv.conv.weight"], views["middle_rpn.reg_conv.conv.bias"]]
        hit = (views, [views[k] for k in VFE_KEYS] + mg)       # the gradient tensors in _flat_params order
        if not accumulate:
            rpn.__dict__["_mg_cache"] = hit
    rpn._ws_release(ws)
    ctx.saved = None          # drop the dense grid etc. now, not when the graph node is collected
    out = hit[1]
    if ctx.anchor:
        # the parameters are not inputs of this Function: their gradients are assigned (or, when a .grad exists, added:
        # what AccumulateGrad would do) here
        if accumulate:
            have = [(p_, g_) for p_, g_ in zip(plist, out) if p_.grad is not None]
            torch._foreach_add_([p_.grad for p_, _ in have], [g_ for _, g_ in have])
            for p_, g_ in zip(plist, out):
                if p_.grad is None:
                    p_.grad = g_
        else:
            for p_, g_ in zip(plist, out):
                p_.grad = g_
        return (None,) * 6
    if accumulate:
        return (None, None, None, None, None) + tuple(out)        # (views of a buffer nobody else holds)
    if rpn.direct_grads:
        # hand the gradients to the parameters directly: returning the (shared) views through autograd would make
        # AccumulateGrad clone all 104 of them every step
        for p_, g_ in zip(plist, out):
            p_.grad = g_
        return (None,) * (5 + len(out))
    return (None, None, None, None, None) + tuple(out)


_DetectorFn._backward_native = staticmethod(_detector_backward_native)


_LOSS_SPECS = {}


def _iou_check(kind, metric, weight):
    if kind is not None:          # (the default path does not import the module)
        from .iou_loss import check_spec
        check_spec(kind, metric, weight)


def loss_spec(cls_loss="bce", focal_alpha=0.25, focal_gamma=2.0, yaw_loss="diff"):
    """-> _lib.VnLossSpec (include/voxelnet_hip.h), checked here on the host: ValueError for what the library
    would answer with VN_EINVAL, before anything is launched.  ("bce", "diff") is all zero: the reference's objective.
    The struct of a checked combination is kept and shared (nothing writes to it): a dictionary look-up per step."""
    key = (cls_loss, focal_alpha, focal_gamma, yaw_loss)
    try:
        return _LOSS_SPECS[key]
    except (KeyError, TypeError):
        pass
    if cls_loss not in ("bce", "focal"):
        raise ValueError(f"cls_loss must be 'bce' or 'focal', not {cls_loss!r}")
    if yaw_loss not in ("diff", "sin"):
        raise ValueError(f"yaw_loss must be 'diff' or 'sin', not {yaw_loss!r}")
    spec = _lib.VnLossSpec(0, int(yaw_loss == "sin"), 0.0, 0.0)
    if cls_loss == "focal":
        fa, ga = float(focal_alpha), float(focal_gamma)
        if not 0.0 <= fa <= 1.0:
            raise ValueError(f"focal_alpha must lie in [0, 1], not {focal_alpha!r}")
        if not (ga == 0.0 or 1.0 <= ga < float("inf")):
            raise ValueError(f"focal_gamma must be 0 or >= 1 (x^gamma and its derivative at x = 0), not {focal_gamma!r}")
        spec.cls_kind, spec.focal_alpha, spec.focal_gamma = _lib.VN_LOSS_FOCAL, fa, ga
    if _lib.load().vn_rpn_loss_spec_check(ctypes.byref(spec)) != 0:
        raise ValueError(f"loss spec refused by the library: {cls_loss!r} {focal_alpha!r} {focal_gamma!r} {yaw_loss!r}")
    _LOSS_SPECS[key] = spec
    return spec


class _LossFn(torch.autograd.Function):
    """model.py:309-352 as two fused passes over the anchor sites (csrc/loss.hip) -> tensor [loss, cls_loss,
    reg_loss, cls_pos_loss_rec, cls_neg_loss_rec].  spec: a _lib.VnLossSpec (loss_spec()), None = the reference's objective"""

    @staticmethod
    def forward(ctx, prob, delta, pos, neg, tgt, alpha, beta, sigma, spec=None):
        _need_cuda(prob, delta, pos, neg, tgt)
        B, _, H, W = prob.shape
        if tuple(delta.shape) != (B, 14, H, W) or tuple(pos.shape) != (B, H, W, 2) or tuple(neg.shape) != (B, H, W, 2) \
                or tuple(tgt.shape) != (B, H, W, 14):
            raise ValueError(f"loss: shapes {tuple(prob.shape)} {tuple(delta.shape)} {tuple(pos.shape)} "
                             f"{tuple(neg.shape)} {tuple(tgt.shape)} do not belong together")
        prob, delta = prob.detach().contiguous().float(), delta.detach().contiguous().float()
        with _lib.on_device(prob.device):
            ws_bytes = _lib.load().vn_rpn_loss_workspace_bytes(B, H, W)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=prob.device)
            out = torch.empty(5, dtype=torch.float32, device=prob.device)
            with E.section("loss_fwd", 4.0 * B * H * W * 34):
                _lib.call("vn_rpn_loss_spec_fwd", prob.data_ptr(), delta.data_ptr(), pos.data_ptr(), neg.data_ptr(), tgt.data_ptr(),
                          B, H, W, alpha, beta, sigma, ws.data_ptr(), ws_bytes, out.data_ptr(), E.stream(),
                          None if spec is None else ctypes.byref(spec))
        ctx.saved = (prob, delta, pos, neg, tgt, ws, (B, H, W, alpha, beta, sigma), spec)
        ctx.set_materialize_grads(False)          # unused outputs arrive as None in backward, not as zero tensors
        return tuple(out[i] for i in range(5))    # five scalars (views of one buffer): loss, cls, reg, cls_pos, cls_neg

    @staticmethod
    def backward(ctx, *gs):
        prob, delta, pos, neg, tgt, ws, (B, H, W, alpha, beta, sigma), spec = ctx.saved
        gs = [None if g is None else g.contiguous().float() for g in gs]
        with _lib.on_device(prob.device):
            d_prob, d_delta = torch.empty_like(prob), torch.empty_like(delta)
            with E.section("loss_bwd", 4.0 * B * H * W * 50):
                _lib.call("vn_rpn_loss_spec_bwd", prob.data_ptr(), delta.data_ptr(), pos.data_ptr(), neg.data_ptr(), tgt.data_ptr(),
                          B, H, W, alpha, beta, sigma, ws.data_ptr(), *[None if g is None else g.data_ptr() for g in gs],
                          d_prob.data_ptr(), d_delta.data_ptr(), E.stream(), None if spec is None else ctypes.byref(spec))
        return d_prob, d_delta, None, None, None, None, None, None, None     # (a trailing None too many is allowed)


_STREAMS = {}


def _shared_stream(device, role):
    """process-wide stream of a role ('side', 'targets') on a device (see RPN3D._side_stream)"""
    key = (torch.device(device), role)
    st = _STREAMS.get(key)
    if st is None:
        st = _STREAMS[key] = torch.cuda.Stream(device=device)
    return st


class RPN3D(nn.Module):
    """model.py:284-362.  forward(x: 7-tuple batch, device) -> 7-tuple like the reference.
    Targets (model.py:309): generated on the device from the batch's label lines x[1] (voxelnet_amd/targets.py,
    csrc/targets.hip), unless `targets=(pos_equal_one, neg_equal_one, targets)` (channels-last arrays as
    utils.generate_targets returns them) is passed or `target_fn` is set.
    anchor_area_threshold: with an int >= 0 the targets generated here are edited by SECOND's anchor mask on the
    target stream, and evaluate / predict hand the batch's mask to the decoder; targets passed in or made by `target_fn` are
    NOT edited (anchor_mask.AnchorMasker is public for those callers)."""

    # the loss's objective.  Class-level defaults: a model pickled before these attributes existed loads
    # without them in its __dict__ and still reads the reference's objective here.
    cls_loss, focal_alpha, focal_gamma, yaw_loss = "bce", 0.25, 2.0, "diff"
    # the rotated-IoU regression term (voxelnet_amd/iou_loss.py): None = off, nothing new is launched
    iou_loss, iou_weight, iou_metric = None, 1.0, "3d"
    last_iou = None          # the latest (L_iou, mean_iou) pair: detached device scalars, no synchronisation
    # how anchors are assigned to ground truths (targets.TargetGenerator(assign=)): "reference" keeps the
    # reference's assignment, "standup" / "rotated" assign by a real IoU, "atss" by every box's own threshold over its
    # atss_top_k nearest anchors per rotation, IoU of kind atss_iou; "simota"  by the network's
    # own predictions — the targets are then generated AFTER detect(), from its detached maps, on the step's dependency chain
    target_assign, atss_top_k, atss_iou = "reference", 9, "rotated"
    ota_q, ota_radius, ota_iou_weight, ota_metric = 10, None, 3.0, "bev"
    # the direction-classifier head (voxelnet_amd/dir_head.py): False = nothing is registered or launched
    dir_head, dir_weight, dir_offset = False, 0.2, math.pi / 4
    last_dir = None          # the latest (L_dir, acc) pair: detached device scalars, no synchronisation
    last_dir_logits = None   # the head's logits (B,2,h,w) of the latest detect(), with the autograd graph in training
    # SECOND's anchor mask (voxelnet_amd/anchor_mask.py): None = off, nothing new is allocated or launched; an
    # int >= 0: an anchor with at most that many voxels over its footprint is ignored by the loss and is never a detection
    anchor_area_threshold = None
    last_anchor_mask = None  # the latest (B,h,w,2) uint8 mask: detached, no synchronisation
    # the IoU-aware confidence head (voxelnet_amd/iou_head.py): False = nothing is registered or launched
    iou_head, iou_head_weight, iou_head_metric, iou_rectify = False, 1.0, "3d", 0.5
    last_iou_head = None     # the latest (L, mae) pair of the head's loss: detached device scalars (last_iou is the regression term's)
    last_iou_logits = None   # the head's logits (B,2,h,w) of the latest detect(), with the autograd graph in training

    def __init__(self, cls_name="Car", alpha=ALPHA, beta=BETA, sigma=SIGMA, *, cls_loss="bce", focal_alpha=0.25, focal_gamma=2.0,
                 yaw_loss="diff", iou_loss=None, iou_weight=1.0, iou_metric="3d", target_assign="reference", dir_head=False,
                 dir_weight=0.2, dir_offset=math.pi / 4, anchor_area_threshold=None, iou_head=False, iou_head_weight=1.0,
                 iou_head_metric="3d", iou_rectify=0.5, atss_top_k=9, atss_iou="rotated", ota_q=10, ota_radius=None,
                 ota_iou_weight=3.0, ota_metric="bev"):
        super().__init__()
        from .targets import check_assign_params
        check_assign_params(target_assign, atss_top_k, atss_iou, ota_q, ota_radius, ota_iou_weight, ota_metric, name="target_assign")
        self.target_assign, self.atss_top_k, self.atss_iou = target_assign, atss_top_k, atss_iou
        self.ota_q, self.ota_radius, self.ota_iou_weight, self.ota_metric = ota_q, ota_radius, ota_iou_weight, ota_metric
        if anchor_area_threshold is not None:
            from .anchor_mask import check_threshold
            self.anchor_area_threshold = check_threshold(anchor_area_threshold)
        self.cls_name, self.alpha, self.beta, self.sigma = cls_name, alpha, beta, sigma
        loss_spec(cls_loss, focal_alpha, focal_gamma, yaw_loss)      # (ValueError here, not at the first step)
        self.cls_loss, self.focal_alpha, self.focal_gamma, self.yaw_loss = cls_loss, focal_alpha, focal_gamma, yaw_loss
        _iou_check(iou_loss, iou_metric, iou_weight)
        self.iou_loss, self.iou_weight, self.iou_metric = iou_loss, iou_weight, iou_metric
        self.dir_head = bool(dir_head)
        if self.dir_head:
            from .dir_head import check_spec
            check_spec(dir_weight, dir_offset)
            self.dir_weight, self.dir_offset = dir_weight, dir_offset
        self.iou_head = bool(iou_head)
        if self.iou_head:
            from .iou_head import check_spec as iou_head_check
            iou_head_check(iou_head_weight, iou_rectify, iou_head_metric)
            self.iou_head_weight, self.iou_head_metric, self.iou_rectify = iou_head_weight, iou_head_metric, iou_rectify
        self.feature_net = FeatureLearningNet(cls_name)
        self.middle_rpn = MiddleConvNet(cls_name, dir_head=self.dir_head, iou_head=self.iou_head)
        self.rpn_output_shape = self.middle_rpn.output_shape
        self.anchors = None      # model.py:295 utils.generate_anchors(): built with the first target generation
        self.target_fn = None    # callable(label, rpn_output_shape) -> (pos, neg, targets)
        self.sparse_first_layer = True   # first Conv3d only at active sites / occupied voxels (same results)
        self.direct_grads = True         # native path: .grad = views of one persistent flat buffer (no clones);
        #                                  set False to accumulate gradients over several backward() calls
        self.native_executor = True      # C++ step executor (csrc/runtime.hip) instead of per-launch Python calls
        self.grad_reducer = None  # parallel.GradAllReducer: bucketed all-reduce overlapped with backward
        self.overlap_wgrad = True # native path: weight-gradient launches on a side stream beside the data-gradient ones
        self.grad_storage = 0     # bf16 mode, native path: vnNetConfig.grad_storage (which step tensors are kept in fp32)

    # Runtime caches kept in the instance __dict__ (ctypes arrays, HIP streams, the ~1.5 GB executor arenas, the flat
    # gradient buffer, device-side target / decode helpers).  They are rebuilt on demand and must not travel with
    # `torch.save(model)` (the reference's checkpoint format, train.py:24/27) or `copy.deepcopy(model)`.
    _RUNTIME_KEYS = ("_side", "_tgt_stream", "_ws_pool", "_flat_grads", "_targets", "_decoder", "_nbt", "_flat_param_list", "_net_ctx",
                     "_named_param_list", "_anchor_t", "_bucket_views", "_mg_cache", "_step_sc", "_nbt_table", "last_iou", "last_dir",
                     "last_dir_logits", "_maskers", "last_anchor_mask", "last_iou_head", "last_iou_logits")

    def __getstate__(self):
        d = self.__dict__.copy()
        for k in self._RUNTIME_KEYS:
            d.pop(k, None)
        d["grad_reducer"] = None          # process groups / comm streams are per process
        return d

    def _net_handle(self, device):
        """the executor context (vn_net_create: fork/join and bucket events) of this module on `device`"""
        device = torch.device(device)
        ctx = self.__dict__.get("_net_ctx")
        if ctx is None or ctx[0] != device:
            if ctx is not None:
                _lib.load().vn_net_destroy(ctx[1])
            h = ctypes.c_void_p()
            with _lib.on_device(device):
                _lib.call("vn_net_create", ctypes.byref(h))
            ctx = (device, h)
            self.__dict__["_net_ctx"] = ctx
        return ctx[1]

    def __del__(self):
        ctx = self.__dict__.get("_net_ctx")
        if ctx is not None:
            try:
                _lib.load().vn_net_destroy(ctx[1])
            except Exception:   # noqa: BLE001 - interpreter shutdown
                pass

    def _side_stream(self, device):
        """HIP stream handle (ctypes) of the side stream for the native executor.  ONE stream per device and role for all
        modules of the process (round 4): the HIP runtime spreads streams over a handful of hardware queues (4 by default)
        in creation order, so a second model's own side stream could share a queue with the training stream and serialise
        against it — measured with the third model of bench.py's parity block: 193 instead of 231 point-clouds/s."""
        st = self.__dict__.get("_side")
        if st is None or st.device != torch.device(device):
            st = _shared_stream(device, "side")
            self.__dict__["_side"] = st
        return ctypes.c_void_p(st.cuda_stream)

    # The native executor's workspace arena (~1.5 GB for the car grid at batch 2) is kept in a small pool owned by
    # the module: handing a buffer of that size back to the caching allocator every step makes it re-hipMalloc
    # (~90 ms) whenever another stream's allocations got in between.
    def _ws_acquire(self, nbytes, device):
        pool = self.__dict__.setdefault("_ws_pool", [])
        for i, t in enumerate(pool):
            if t.numel() >= nbytes and t.device == device:
                return pool.pop(i)
        return torch.empty(nbytes, dtype=torch.uint8, device=device)

    def _ws_release(self, ws):
        pool = self.__dict__.setdefault("_ws_pool", [])
        if len(pool) < 2 and all(t is not ws for t in pool):
            pool.append(ws)

    def _target_generator(self, device):
        from .targets import TargetGenerator
        gen = self.__dict__.get("_targets")
        # TargetGenerator's arguments after the device and the anchors (None: the class's grid), as they are NOW — they may
        # be set after construction —: its .key.  (With the direction head the labels keep their heading: its target is the
        # bin of the box's yaw)
        key = (self.cls_name, self.target_assign, None, None, bool(self.dir_head), self.atss_top_k, self.atss_iou, self.ota_q,
               self.ota_radius, self.ota_iou_weight, self.ota_metric)
        if gen is None or (gen.device, gen.key) != (torch.device(device), key):
            gen = TargetGenerator(key[0], device, None, *key[1:])
            # the maps the network EMITS, not rpn_output_shape: for Pedestrian / Cyclist that attribute repeats the anchor
            # grid (100 x 120, as the reference has it) while block 1 does not stride and the maps are 200 x 240
            g, s = grid_config(self.cls_name), self.middle_rpn._block1_stride
            emitted = (g.H // s, g.W // s)
            if tuple(gen.shape) != emitted:
                # (the reference has the same mismatch for Pedestrian / Cyclist: its loss cannot run)
                raise _lib.VoxelnetHipError(f"anchor grid {tuple(gen.shape)} != RPN output {emitted}")
            self.__dict__["_targets"] = gen
            self.anchors = gen.anchors
        return gen

    def _anchor_masker(self, device, anchors):
        """the anchor_mask.AnchorMasker of `anchors` (the target generator's or a decoder's (h,w,2,7) array) on this module's
        voxel grid at anchor_area_threshold as it is now (like cls_loss it may be set after construction); a few are kept,
        by the array they were built from: the cell rectangles are host work per anchor set"""
        from .anchor_mask import AnchorMasker, check_threshold
        thr, grid, device = check_threshold(self.anchor_area_threshold), self.feature_net._grid, torch.device(device)
        cache = self.__dict__.setdefault("_maskers", {})
        hit = cache.get(id(anchors))
        if hit is None or hit[0] is not anchors or hit[1].device != device or hit[1].threshold != thr or hit[1].grid != grid:
            if len(cache) >= 4:
                cache.clear()
            hit = cache[id(anchors)] = (anchors, AnchorMasker(self.cls_name, device, anchors=anchors, threshold=thr, grid=grid))
        return hit[1]

    def _mask_targets(self, targets, voxel_coordinates, main):
        """anchor_area_threshold set, targets the module generated itself: the anchors without voxels under them become
        ignored — pos = neg = 0 in place (vn_anchor_mask) — on the CURRENT stream, the target stream, which is first ordered
        after `main`, the stream the batch's coordinates are ready on (None: they are ready on this one).  Caller-supplied
        targets and a target_fn's are never edited."""
        pos, neg = targets[0], targets[1]
        dev = pos.device
        cur = _lib.current_stream(dev)
        if main is not None and main != cur:
            with torch.cuda.stream(main):
                coord = _batch_cat(voxel_coordinates, torch.int64)
            cur.wait_stream(main)
            coord.record_stream(cur)
        else:
            coord = _batch_cat(voxel_coordinates, torch.int64)
        masker = self._anchor_masker(dev, self._target_generator(dev).anchors)
        self.last_anchor_mask = masker.mask(coord, len(voxel_coordinates), pos=pos, neg=neg)
        return targets

    def _decode_mask(self, dec, voxel_coordinates, device):
        """the (B,h,w,2) uint8 mask of a batch for the decoder `dec` (its anchors), on the current stream"""
        coord = _batch_cat(_parts_to(voxel_coordinates, device), torch.int64)
        if not coord.is_cuda:
            raise _lib.VoxelnetHipError("anchor_area_threshold: the voxel coordinates must live on a HIP device (no CPU path)")
        self.last_anchor_mask = self._anchor_masker(coord.device, dec.anchors).mask(coord, len(voxel_coordinates))
        return self.last_anchor_mask

    def _tta_decode(self, x, device, dec, kw, top_k, tta, own=None):
        """One batch through test-time augmentation (tta.TestTimeAugment) -> decode_device's (boxes, scores,
        counts) on the device.  Per view: the identity view takes the batch's own voxel buffers x[2] / x[4] (or `own`, its
        (prob, delta, head keywords) when the caller has run it already); every other view uploads the raw cloud x[6][b][:, :4],
        crops it when tta.fov_calib_dir is set, moves it by vn_augment_compose, voxelizes it on the model's grid and runs
        detect; candidates_device with THAT view's direction / IoU logits and anchor mask.  Then tta.merge_pools, nms_device
        on the merged pool and tta.vote_device (tta.vote None: a gather of the kept rows).  kw: decode_device's keyword
        arguments score_thres, nms, nms_thres, pre_nms_top_k, layout and soft_nms (predict.soft_nms_device on the
        merged pool in place of nms_device; needs tta.vote None).  Must run in eval mode under no_grad."""
        from . import predict as PR
        from .tta import TestTimeAugment, merge_pools, vote_device
        from .voxelize import voxelize_device_async
        if not isinstance(tta, TestTimeAugment):
            raise ValueError(f"tta must be a tta.TestTimeAugment, not {tta!r}")
        kw = dict(kw)
        score_thres, nms = kw.pop("score_thres", PR.SCORE_THRES), kw.pop("nms", "standup")
        nms_thres, pre, layout = kw.pop("nms_thres", PR.NMS_THRES), kw.pop("pre_nms_top_k", None), kw.pop("layout", None)
        soft = kw.pop("soft_nms", None)
        if kw:
            raise ValueError(f"tta: the decode may set score_thres, nms, nms_thres, pre_nms_top_k, layout and soft_nms, not {sorted(kw)}")
        if soft is not None:
            if not isinstance(soft, PR.SoftNMS):
                raise ValueError(f"soft_nms must be a predict.SoftNMS, not {soft!r}")
            if nms != "rotated":
                raise ValueError(f"soft_nms decays by the rotated IoU; nms must be 'rotated', not {nms!r}")
            if tta.vote is not None:
                raise ValueError("tta: soft_nms with a vote is not defined (the vote's cluster around a soft-kept row); pass "
                                 "TestTimeAugment(vote=None)")
        pre = top_k if pre is None else pre
        V = len(tta.views)
        if not (isinstance(pre, (int, np.integer)) and 1 <= pre and pre * V <= _lib.VN_DETECT_MAX_PRE):
            raise ValueError(f"tta: pre_nms_top_k * len(views) = {pre!r} * {V} must be in [1, {_lib.VN_DETECT_MAX_PRE}]")
        raw = x[6] if len(x) > 6 else None
        if any(not v.identity for v in tta.views) and (raw is None or len(raw) == 0 or any(c is None for c in raw)):
            raise _lib.VoxelnetHipError("tta: every view but the identity needs the frames' raw clouds (x[6])")
        lkw = {} if layout is None else {"layout": layout}
        grid, pools, held = self.feature_net._grid, [], []
        for view in tta.views:
            if view.identity and own is not None:
                prob, delta, hkw = own
                coords = _parts_to(x[4], device) if self.anchor_area_threshold is not None else None
            else:
                if view.identity:
                    feats, coords = _parts_to(x[2], device), _parts_to(x[4], device)
                else:
                    handles = []
                    for b, cloud in enumerate(raw):
                        pts, keep = tta.view_points(view, cloud, x[0][b], x[5][b] if len(x) > 5 and x[5] is not None else None, device)
                        handles.append(voxelize_device_async(pts, grid, b, coord_cols=4))
                        held.append((pts, keep))
                    feats, coords = [], []
                    for h in handles:
                        f, c, _ = h.result()
                        feats.append(f)
                        coords.append(c)
                prob, delta = self.detect(feats, coords)
                hkw = self._dir_decode(lkw, dec)          # this view's direction / IoU logits
            if self.anchor_area_threshold is not None:
                hkw = dict(hkw, anchor_mask=self._decode_mask(dec, coords, device))          # and this view's occupancy
            pools.append(dec.candidates_device(prob, delta, score_thres, int(pre), **hkw))
        mb, ms, src, mc = merge_pools([p[0] for p in pools], [p[1] for p in pools], [p[3] for p in pools], tta.views)
        if soft is not None:
            keep, ks, kc = PR.soft_nms_device(mb, ms, mc, soft, top_k, min_score=float(score_thres))
            return PR.gather_kept(mb, ms, keep, kc, keep_scores=ks)
        keep, kc = PR.nms_device(mb, mc, nms, nms_thres, top_k)
        if tta.vote is None:
            return PR.gather_kept(mb, ms, keep, kc)
        return vote_device(mb, ms, mc, keep, kc, tta.vote, src=src, rows_per_view=int(pre), n_views=V)[:3]

    def predict(self, data, probs, deltas, summary=False, visual=False, decode=None, tta=None):
        """model.py:364-441 without the drawing branches: -> (tag, ret_box_3d_score), one array per sample of
        [cls_name, x, y, z, h, w, l, r, score] rows (strings, as np.concatenate makes them at model.py:389-394).
        Decoding, score filter and NMS run on the device (voxelnet_amd/predict.py, csrc/predict.hip).  decode: a dict of
        BoxDecoder keyword arguments (None: the reference's tail; predict.TRAINED_DECODE for a model trained here).
        tta: a tta.TestTimeAugment — probs / deltas (and the heads' logits of the detect() that made them)
        serve the identity view, every other view is run from the raw clouds data[6]; the module must be in eval mode."""
        if summary or visual:
            raise NotImplementedError("the summary / visual branches of RPN3D.predict draw with OpenCV (model.py:396-439): "
                                      "outside the accelerated path")
        dec = self._box_decoder(probs.device)
        if tta is not None:
            if self.training:
                raise _lib.VoxelnetHipError("predict: tta runs further forwards; put the module in eval mode first")
            kw = dict(decode or {})
            from .predict import NMS_POST_TOPK
            top_k = kw.pop("top_k", NMS_POST_TOPK)
            lkw = {"layout": kw["layout"]} if "layout" in kw else {}
            with torch.no_grad():
                boxes, scores, counts = self._tta_decode(data, probs.device, dec, kw, top_k, tta,
                                                         own=(probs, deltas, self._dir_decode(lkw, dec)))
            cnt, bh, sh = counts.cpu().numpy(), boxes.cpu().numpy(), scores.cpu().numpy()
            out = [np.concatenate([np.tile(self.cls_name, int(cnt[b]))[:, np.newaxis], bh[b, :cnt[b]], sh[b, :cnt[b], np.newaxis]],
                                  axis=-1) for b in range(len(cnt))]
            return data[0], out
        kw = self._dir_decode(dict(decode or {}), dec)
        if self.anchor_area_threshold is not None:
            # (the mask comes from the voxel coordinates of the batch the maps were made from, data[4])
            if len(data) < 5 or data[4] is None:
                raise _lib.VoxelnetHipError("predict: anchor_area_threshold needs the batch's voxel coordinates (data[4])")
            kw["anchor_mask"] = self._decode_mask(dec, data[4], probs.device)
        ret_box_3d, ret_score = dec(probs, deltas, **kw)
        out = []
        for boxes_3d, scores in zip(ret_box_3d, ret_score):
            out.append(np.concatenate([np.tile(self.cls_name, len(boxes_3d))[:, np.newaxis], boxes_3d,
                                       scores[:, np.newaxis]], axis=-1))
        return data[0], out

    def _dir_decode(self, kw, dec=None):
        """`kw` (BoxDecoder keyword arguments) with the direction head's logits of the latest detect() and its offset added
        when the head is on; the decode then has to read the maps by site (predict.TRAINED_DECODE).  The IoU-aware head's
        logits and iou_rectify travel the same way, under the same rule."""
        if self.iou_head:
            layout = kw.get("layout", dec.layout if dec is not None else "flat")
            if layout != "site":
                raise ValueError(f"iou_head: the IoU-aware head's logits are laid out by site; decode with layout='site' "
                                 f"(predict.TRAINED_DECODE), not {layout!r}")
            if self.last_iou_logits is None:
                raise _lib.VoxelnetHipError("iou_head: no logits yet — decode after detect() / forward()")
            kw = dict(kw, iou_logits=self.last_iou_logits.detach(), iou_rectify=float(self.iou_rectify))
        if not self.dir_head:
            return kw
        layout = kw.get("layout", dec.layout if dec is not None else "flat")
        if layout != "site":
            raise ValueError(f"dir_head: the direction head's logits are laid out by site; decode with layout='site' "
                             f"(predict.TRAINED_DECODE), not {layout!r}")
        if self.last_dir_logits is None:
            raise _lib.VoxelnetHipError("dir_head: no logits yet — decode after detect() / forward()")
        return dict(kw, dir_logits=self.last_dir_logits.detach(), dir_offset=float(self.dir_offset))

    def _box_decoder(self, device):
        from .predict import BoxDecoder
        dec = self.__dict__.get("_decoder")
        if dec is None or dec.device != device:
            dec = BoxDecoder(self.cls_name, device)
            self.__dict__["_decoder"] = dec
            self.anchors = dec.anchors
        return dec

    def evaluate(self, batches, device, evaluator=None, decoder=None, decode=None, ema=None, calib=None, tta=None):
        """The validation loop a user would otherwise write around `predict`: every batch tuple of `batches` (the
        7-tuples forward takes; x[1] = label lines) goes through an eval-mode, no_grad forward, BoxDecoder.decode_device
        and evaluator.update — the maps, the decoded boxes and the matching stay on the device, nothing is waited for
        until the caller asks the returned evaluator to compute().  evaluator: an evaluate.DetectionEvaluator (default:
        a new one for this class); decoder: a predict.BoxDecoder (default: the module's own, full anchor grid); decode: a dict of
        BoxDecoder.decode_device keyword arguments (e.g. predict.EVAL_DECODE: a pre-NMS top-K and the rotated NMS; None:
        the reference's tail); the post-NMS cap is always evaluator.top_k.  ema: an ema.ModelEMA of this module — the loop then
        runs inside `ema.applied()`, i.e. scores the averaged weights (and averaged running statistics); the eval forward
        reads the parameters afresh at every call (weights are packed per forward, nothing is cached from their values), so
        the exchange needs no invalidation.  The module is back in the mode it was in afterwards, and holds its own weights.
        calib: None — the protocol of DESIGN.md §1b, as above; or "mean", a directory of <tag>.txt KITTI calibration files,
        or a callable tag -> (P2, Tr_velo_to_cam, R0_rect): KITTI's image-plane protocol (§1b-bis).  The evaluator is then an
        evaluate.KittiDetectionEvaluator (default: a new one); x[0]'s tags pick each frame's calibration and are
        remembered for its write_results.
        tta: None — every path above exactly as it is; or a tta.TestTimeAugment: every batch is run once per
        view from its raw clouds x[6], the views' candidates are merged, suppressed and voted on the device (`_tta_decode`);
        `decode` may then set score_thres, nms, nms_thres, pre_nms_top_k (times the number of views <= 4096), layout and
        soft_nms (a predict.SoftNMS; with it tta.vote must be None)."""
        from .evaluate import DetectionEvaluator, KittiDetectionEvaluator, calib_source
        device = torch.device(device)
        calib_of = None
        if calib is not None:
            calib_of = calib_source(calib)
            if evaluator is None:
                evaluator = KittiDetectionEvaluator(self.cls_name, device)
            elif not isinstance(evaluator, KittiDetectionEvaluator):
                raise ValueError("evaluate: `calib` needs an evaluate.KittiDetectionEvaluator")
        if evaluator is None:
            evaluator = DetectionEvaluator(self.cls_name, device)
        dec = self._box_decoder(device) if decoder is None else decoder
        kw = dict(decode or {})
        if "top_k" in kw:
            raise ValueError("evaluate: the post-NMS cap is evaluator.top_k; `decode` may not set top_k")
        if ema is not None and ema.model is not self:
            raise ValueError("evaluate: `ema` averages another module")
        if self.dir_head and kw.get("layout", dec.layout) != "site":
            raise ValueError("evaluate: with dir_head the decode must read the maps by site: decode=predict.TRAINED_DECODE")
        if self.iou_head and kw.get("layout", dec.layout) != "site":
            raise ValueError("evaluate: with iou_head the decode must read the maps by site: decode=predict.TRAINED_DECODE")
        was_training = self.training
        self.eval()
        try:
            with torch.no_grad(), (ema.applied() if ema is not None else contextlib.nullcontext()):
                for x in batches:
                    if tta is not None:
                        det = self._tta_decode(x, device, dec, kw, evaluator.top_k, tta)
                        if calib_of is None:
                            evaluator.update(*det, x[1])
                        else:
                            evaluator.update(*det, x[1], calibs=[calib_of(tag) for tag in x[0]], tags=list(x[0]))
                        continue
                    prob, delta = self.detect(_parts_to(x[2], device), _parts_to(x[4], device))
                    if self.anchor_area_threshold is None:
                        det = dec.decode_device(prob, delta, top_k=evaluator.top_k, **self._dir_decode(kw, dec))
                    else:                         # (an anchor without voxels under it is never a detection)
                        det = dec.decode_device(prob, delta, top_k=evaluator.top_k, **self._dir_decode(kw, dec),
                                                anchor_mask=self._decode_mask(dec, x[4], device))
                    if calib_of is None:
                        evaluator.update(*det, x[1])
                    else:
                        evaluator.update(*det, x[1], calibs=[calib_of(tag) for tag in x[0]], tags=list(x[0]))
        finally:
            self.train(was_training)
        return evaluator

    def _named_params(self):
        """list(self.named_parameters()), cached (the Parameter objects are stable; see _flat_params)"""
        np_ = self.__dict__.get("_named_param_list")
        if np_ is None:
            np_ = list(self.named_parameters())
            self.__dict__["_named_param_list"] = np_
        return np_

    def _anchor(self, device):
        """the one-element leaf that stands for all parameters in the autograd graph of the native path (_DetectorFn)"""
        a = self.__dict__.get("_anchor_t")
        if a is None or a.device != torch.device(device):
            a = torch.zeros(1, device=device, requires_grad=True)
            self.__dict__["_anchor_t"] = a
        return a

    def _flat_params(self):
        """the 8 VFE + 96 middle/RPN parameters in the executor's order (the Parameter objects are stable: `.to()` and
        `load_state_dict` change their data in place), cached: the module walk costs ~0.15 ms of host time per call"""
        fp = self.__dict__.get("_flat_param_list")
        if fp is None:
            fp = _vfe_weights(self.feature_net) + _collect_middle(self.middle_rpn)[3]
            self.__dict__["_flat_param_list"] = fp
        return fp

    def _tick(self):
        """num_batches_tracked += 1 of all 25 BatchNorms (nn.BatchNorm*.forward in train mode) as ONE launch, on the side
        stream: nothing in the step depends on the counters, so they do not sit on the main chain."""
        if not self.training:
            return
        dev = self.middle_rpn.prob_conv.conv.weight.device
        ctrs = self.__dict__.get("_nbt")
        if ctrs is None or ctrs[0].device != dev:
            ctrs = [m.num_batches_tracked for m in self.modules()
                    if isinstance(m, (nn.BatchNorm1d, nn.BatchNorm2d, nn.BatchNorm3d))]
            self.__dict__["_nbt"] = ctrs
        side = self.__dict__.get("_side") if self.overlap_wgrad and dev.type == "cuda" else None
        if side is None:
            torch._foreach_add_(ctrs, 1)
            return
        side.wait_stream(torch.cuda.current_stream())          # (after whatever wrote the counters before, e.g. load_state_dict)
        with torch.cuda.stream(side):
            torch._foreach_add_(ctrs, 1)
        if not torch.is_grad_enabled():                        # no backward will join the side stream: do it here
            torch.cuda.current_stream().wait_stream(side)

    def detect(self, voxel_features, voxel_coordinates):
        """feature_net + middle_rpn (model.py:305-306), fused."""
        bs = len(voxel_features)
        feature, coord = _batch_cat(voxel_features, torch.float32), _batch_cat(voxel_coordinates, torch.int64)
        flat = self._flat_params()
        if self.dir_head:
            self._dir_check(_mode())
            flat = flat + _dir_params(self.middle_rpn)
        if self.iou_head:
            self._iou_head_check(_mode())
            flat = flat + _iou_params(self.middle_rpn)
        if (self._native_ok(_mode()) and self.training and self.direct_grads and torch.is_grad_enabled() and feature.is_cuda
                and self._all_need_grad(flat)):
            prob, reg = _DetectorFn.apply(feature, coord, bs, self, self.training, self._anchor(feature.device))
        else:
            if not torch.is_grad_enabled():
                # (an autograd Function's needs_input_grad follows requires_grad, not the grad mode: without this, an eval
                # forward under no_grad — the validation / predict call — left the native executor for the per-layer path)
                flat = [p.detach() for p in flat]
            out = _DetectorFn.apply(feature, coord, bs, self, self.training, *flat)
            prob, reg = out[0], out[1]
            if self.dir_head:
                self.last_dir_logits = out[2]
            if self.iou_head:
                self.last_iou_logits = out[-1]
        self._tick()
        return prob, reg

    def _iou_head_check(self, mode):
        """_dir_check for the IoU-aware head (out of scope): the fp32x3 mode and a gradient reducer"""
        if mode == "fp32x3" or E.X3["on"]:
            raise ValueError("iou_head: the fp32x3 mode is not supported with the IoU-aware head; use 'bf16' or 'fp32'")
        if self.grad_reducer is not None:
            raise ValueError("iou_head: a grad_reducer is not supported with the IoU-aware head: the DDP bucket plan does not "
                             "know its two parameters")

    def _dir_check(self, mode):
        """ValueError for what the direction head does not run with (out of scope): the fp32x3 mode, and a
        gradient reducer, whose bucket plan does not know the head's two parameters"""
        if mode == "fp32x3" or E.X3["on"]:
            raise ValueError("dir_head: the fp32x3 mode is not supported with the direction head; use 'bf16' or 'fp32'")
        if self.grad_reducer is not None:
            raise ValueError("dir_head: a grad_reducer is not supported with the direction head: the DDP bucket plan does not "
                             "know its two parameters")

    def _native_ok(self, mode):
        """ONE predicate for "this call runs on the native executor" (csrc/runtime.hip: grids whose depth folds to 2 —
        D = 9 ... 12 —, bf16 / fp32 modes), used by detect() to pick the one-tensor call and by _DetectorFn.forward to pick the
        path: every other configuration (bf16x3, other depths, native_executor = False, dir_head = True: the direction head
        rides on the per-layer orchestration) trains through the per-layer orchestration with the 104
        parameters (and the head's two) as autograd inputs."""
        return (bool(self.native_executor) and not self.dir_head and not self.iou_head          # (iou_head: DESIGN.md 1l, likewise)
                and not E.is_split(mode) and 9 <= self.feature_net._grid.D <= 12)

    def _all_need_grad(self, flat):
        return all(p.requires_grad for p in flat)

    def _loss_spec(self):
        """the vnLossSpec of cls_loss / focal_alpha / focal_gamma / yaw_loss as they are now (they may be set after construction)"""
        return loss_spec(self.cls_loss, self.focal_alpha, self.focal_gamma, self.yaw_loss)

    def _iou_spec(self):
        """None, or the checked (kind, metric, weight) of iou_loss / iou_metric / iou_weight as they are now (like cls_loss
        they may be set after construction)"""
        if self.iou_loss is None:
            return None
        _iou_check(self.iou_loss, self.iou_metric, self.iou_weight)
        return self.iou_loss, self.iou_metric, float(self.iou_weight)

    def loss(self, prob_out, delta_out, pos_equal_one, neg_equal_one, targets):
        """model.py:310-352 -> (loss, cls_loss, reg_loss, cls_pos_loss_rec, cls_neg_loss_rec), fused (csrc/loss.hip); with
        cls_loss="focal" / yaw_loss="sin" the objective of DESIGN.md 1e, same five outputs.  With iou_loss set,
        iou_weight * L_iou (the anchors are the target generator's) is added to loss and to reg_loss and
        the pair (L_iou, mean_iou) is kept, detached, as self.last_iou.  With dir_head on, dir_weight * L_dir (DESIGN.md 1i;
        the logits are last_dir_logits of the detect() before) is added to loss and to cls_loss, and (L_dir, acc) is kept,
        detached, as self.last_dir.  With iou_head on, iou_head_weight * L (the logits are last_iou_logits, the
        target is the IoU of the box delta_out decodes to, a constant) is added to loss and to cls_loss, and (L, mae) is kept,
        detached, as self.last_iou_head."""
        dev = prob_out.device
        spec, iou = self._loss_spec(), self._iou_spec()

        def f32(a):
            if torch.is_tensor(a) and a.dtype == torch.float32 and a.device == dev and a.is_contiguous():
                return a
            return (a if torch.is_tensor(a) else torch.from_numpy(np.asarray(a))).to(dev).float().contiguous()
        pos, tgt = f32(pos_equal_one), f32(targets)
        out = _LossFn.apply(prob_out, delta_out, pos, f32(neg_equal_one), tgt,
                            float(self.alpha), float(self.beta), float(self.sigma), spec)
        if iou is None and not self.dir_head and not self.iou_head:
            return out
        gen = self._target_generator(dev)
        if gen.n_anchors != delta_out.shape[2] * delta_out.shape[3] * 2:
            raise _lib.VoxelnetHipError(f"iou_loss / dir_head: the target generator's anchor grid {tuple(gen.shape)} is not the "
                                        f"regression map's {tuple(delta_out.shape[2:])}")
        if iou is not None:
            from .iou_loss import rpn_iou_loss
            l_iou, mean_iou = rpn_iou_loss(delta_out, pos, tgt, gen._anchors_dev, iou[0], iou[1])
            self.last_iou = (l_iou.detach(), mean_iou)
            term = iou[2] * l_iou
            out = (out[0] + term, out[1], out[2] + term) + tuple(out[3:])
        if self.dir_head:
            from .dir_head import check_spec, rpn_dir_loss
            check_spec(self.dir_weight, self.dir_offset)
            logits = self.last_dir_logits
            if logits is None or logits.shape[0] != delta_out.shape[0] or tuple(logits.shape[2:]) != tuple(delta_out.shape[2:]):
                raise _lib.VoxelnetHipError("dir_head: loss() needs the logits of the detect() that produced these maps")
            l_dir, acc = rpn_dir_loss(logits, pos, tgt, gen._anchors_dev, float(self.dir_offset))
            self.last_dir = (l_dir.detach(), acc)
            term = float(self.dir_weight) * l_dir
            out = (out[0] + term, out[1] + term) + tuple(out[2:])
        if self.iou_head:
            # iou_head_weight * L joins loss and cls_loss; the target is a constant, delta_out gets no gradient
            from .iou_head import check_spec as iou_head_check, rpn_iou_head_loss
            iou_head_check(self.iou_head_weight, self.iou_rectify, self.iou_head_metric)
            logits = self.last_iou_logits
            if logits is None or logits.shape[0] != delta_out.shape[0] or tuple(logits.shape[2:]) != tuple(delta_out.shape[2:]):
                raise _lib.VoxelnetHipError("iou_head: loss() needs the logits of the detect() that produced these maps")
            l_head, mae = rpn_iou_head_loss(logits, delta_out, pos, tgt, gen._anchors_dev, self.iou_head_metric)
            self.last_iou_head = (l_head.detach(), mae)
            term = float(self.iou_head_weight) * l_head
            out = (out[0] + term, out[1] + term) + tuple(out[2:])
        return out

    # ---- one library call per train step (vn_net_step) ------------------------------------------------------------------
    def _step_scratch(self, dev, K, T, B, mode, hf, wf):
        """scratch buffers of vn_net_step, kept on the module and grown with K (nothing here is seen by the caller; the
        step's streams are joined at its end, so the next step may overwrite them)"""
        sc = self.__dict__.get("_step_sc")
        cap = (K + 4095) // 4096 * 4096
        lib = _lib.load()
        key = (dev, T, B, mode, hf, wf)
        if sc is None or sc["key"] != key or sc["cap"] < K:
            cap = max(cap, sc["cap"] if sc is not None and sc["key"] == key else 0)
            sc = {"key": key, "cap": cap}
            sc["vfe_ws_bytes"] = lib.vn_vfe_workspace_bytes(cap, T)
            sc["vfe_ws"] = torch.empty(sc["vfe_ws_bytes"], dtype=torch.uint8, device=dev)
            sc["vw"] = torch.empty((cap, 128), dtype=torch.float32, device=dev)
            sc["vw_rows"] = torch.empty((cap, 128), dtype=torch.bfloat16, device=dev) if mode == "bf16" else sc["vw"]
            sc["d_vw"] = torch.empty((cap, 128), dtype=torch.float32, device=dev)
            sc["stats"] = torch.empty(320, dtype=torch.float32, device=dev)
            sc["heads_w"] = torch.empty((16, 768), dtype=torch.float32, device=dev)
            sc["heads_b"] = torch.empty(16, dtype=torch.float32, device=dev)
            sc["d_prob"] = torch.empty((B, 2, hf, wf), dtype=torch.float32, device=dev)
            sc["d_reg"] = torch.empty((B, 14, hf, wf), dtype=torch.float32, device=dev)
            sc["loss_ws_bytes"] = lib.vn_rpn_loss_workspace_bytes(B, hf, wf)
            sc["loss_ws"] = torch.empty(sc["loss_ws_bytes"], dtype=torch.uint8, device=dev)
            sc["one"] = torch.ones(1, dtype=torch.float32, device=dev)
            sc["args"] = _lib.VnStep()
            self.__dict__["_step_sc"] = sc
        return sc

    def _step_fused_ok(self, mode, optimizer, targets=None):
        """whether train_step may take the one library call.  Under target_assign "simota" the module's own targets need the
        forward's maps, which vn_net_step does not hand out between its forward and its loss: only a step that
        is handed its targets can."""
        from .optim import ClipAdamW, ClipSGD
        red = self.grad_reducer
        return (self._native_ok(mode) and (self.target_assign != "simota" or targets is not None)
                and self.training and self.direct_grads and self.overlap_wgrad and self.sparse_first_layer
                and torch.is_grad_enabled() and self.target_fn is None and E.SECTIONS is None and self.iou_loss is None
                and not (int(self.grad_storage) & 16)
                and (red is None or (red.comm_stream is not None and HEADS_W in _grad_views(self)))
                and (optimizer is None or isinstance(optimizer, (ClipSGD, ClipAdamW))))

    def train_step(self, x, device, optimizer=None, targets=None):
        """One training step — `out = model(x, device); out[2].backward(); clip_grad_norm_; optimizer.step()`
        (model.py:298-362 and train.py:148-154) — as ONE library call (vn_net_step, csrc/runtime.hip): same kernels, same
        order, same streams, bit-identical results; what goes is the host's work between the calls (two autograd Functions,
        the engine's hand-over to its device thread, ~15 tensor allocations, ~12 ctypes calls).
        Returns the tuple forward() returns (tensors without an autograd graph: the backward has already run); the
        parameters' .grad are set as backward() leaves them.  optimizer: a ClipSGD (its update runs inside the call when no
        gradient reducer is attached, after the reducer's exchange otherwise), a ClipAdamW (the call runs without a parameter
        update and optimizer.step() follows on the same stream, after the reducer's exchange) or None (no update).  With a
        weight average attached to the optimizer (optim.attach_ema) a ClipSGD steps after the call too, same parameters.
        Whatever the fused call does not cover — per-layer orchestration, eval mode, target_fn, gradient accumulation, a
        reducer without a communication stream, bench.py's per-section timer, the rotated-IoU term (iou_loss set: it is
        not part of vnStep), the direction head (dir_head=True: it runs on the per-layer orchestration, outside
        the native executor), the IoU-aware head (iou_head=True, likewise), the SimOTA assignment
        without targets= (target_assign="simota": its targets come from the forward's own maps) — takes the
        separate calls, same results."""
        from .optim import ClipSGD
        mode = _mode()
        spec = self._loss_spec()            # (checked before anything is launched)
        self._iou_spec()
        fused = self._step_fused_ok(mode, optimizer, targets)
        plist = self._flat_params() if fused else None
        if fused and (not self._all_need_grad(plist) or any(p.grad is not None for p in plist)):
            fused = False            # (frozen parameters / accumulation into existing .grad: autograd's business)
        label, voxel_features, voxel_coordinates = x[1], x[2], x[4]
        if fused and not (targets is not None or label is not None):
            fused = False
        if not fused:
            out = self(x, device, targets=targets)
            out[2].backward()
            if self.grad_reducer is not None:
                self.grad_reducer.finish(self._named_params())
            if optimizer is not None:
                optimizer.step()
            return out
        voxel_features = _parts_to(voxel_features, device)
        voxel_coordinates = _parts_to(voxel_coordinates, device)
        dev = voxel_features[0].device
        if not voxel_features[0].is_cuda:
            raise _lib.VoxelnetHipError("RPN3D.train_step: the voxel buffers must live on a HIP device (no CPU path)")
        red = self.grad_reducer
        with _lib.on_device(dev):
            ts = None
            if targets is None:
                ts = self.__dict__.get("_tgt_stream")
                if ts is None or ts.device != dev:
                    from .voxelize import pipeline_stream
                    ts = self.__dict__["_tgt_stream"] = pipeline_stream(dev)
                main = _lib.current_stream(dev) if self.anchor_area_threshold is not None else None
                with torch.cuda.stream(ts):
                    targets = self._target_generator(dev)(label)
                    if main is not None:          # (the edited maps are the pos / neg that go into vnStep)
                        targets = self._mask_targets(targets, voxel_coordinates, main)
            else:
                def f32(a):
                    if torch.is_tensor(a) and a.dtype == torch.float32 and a.device == dev and a.is_contiguous():
                        return a
                    return (a if torch.is_tensor(a) else torch.from_numpy(np.asarray(a))).to(dev).float().contiguous()
                targets = tuple(f32(a) for a in targets)
            pos, neg, tgt = targets
            B = len(voxel_features)
            feature, coord = _batch_cat(voxel_features, torch.float32), _batch_cat(voxel_coordinates, torch.int64)
            K, T = feature.shape[0], feature.shape[1]
            fn, mid = self.feature_net, self.middle_rpn
            D, H, W = fn._grid.dims
            hf, wf = H // mid._block1_stride, W // mid._block1_stride
            if tuple(pos.shape) != (B, hf, wf, 2) or tuple(neg.shape) != (B, hf, wf, 2) or tuple(tgt.shape) != (B, hf, wf, 14):
                raise ValueError(f"train_step: target shapes {tuple(pos.shape)} {tuple(neg.shape)} {tuple(tgt.shape)} do not "
                                 f"belong to a batch of {B} on a {hf} x {wf} map")
            cfg = _lib.VnNetConfig(B, D, H, W, mid._block1_stride, {"bf16": 0, "fp32": 1, "fp32x3": 2}[mode], 1, 1, 0, 0, 0, 0)
            cfg.grad_storage = int(self.grad_storage) & (16 if E.is_f32_storage(mode) else 15)
            cfg.bucket_events = int(red is not None)
            lib = _lib.load()
            ws_bytes = lib.vn_net_workspace_bytes(ctypes.byref(cfg), K)
            if ws_bytes == 0:
                raise _lib.VoxelnetHipError("vn_net_workspace_bytes: unsupported network configuration")
            ws = self._ws_acquire(ws_bytes, dev)
            sc = self._step_scratch(dev, K, T, B, mode, hf, wf)
            views = _grad_views(self)
            arr, garr = _native_layer_arrays(mid, views)
            vp = [p for p in plist[:8]]
            bufs = fn._bufs()
            hp = plist[-4:]
            prob = torch.empty((B, 2, hf, wf), dtype=torch.float32, device=dev)
            reg = torch.empty((B, 14, hf, wf), dtype=torch.float32, device=dev)
            loss5 = torch.empty(5, dtype=torch.float32, device=dev)
            a = sc["args"]
            a.feature, a.coord, a.K, a.T = feature.data_ptr(), coord.data_ptr(), K, T
            a.bn_momentum, a.bn_eps = E.BN_MOMENTUM, E.BN_EPS
            a.vfe = _lib.VnVfeWeights(vp[0].data_ptr(), vp[1].data_ptr(), vp[2].data_ptr(), vp[3].data_ptr(), bufs[0].data_ptr(),
                                      bufs[1].data_ptr(), vp[4].data_ptr(), vp[5].data_ptr(), vp[6].data_ptr(), vp[7].data_ptr(),
                                      bufs[2].data_ptr(), bufs[3].data_ptr())
            a.vfe_grads = _lib.VnVfeGrads(*[views[k].data_ptr() for k in VFE_KEYS])
            a.vfe_ws, a.vfe_ws_bytes = sc["vfe_ws"].data_ptr(), sc["vfe_ws_bytes"]
            a.voxelwise, a.vfe_stats, a.vw_rows, a.d_voxelwise = (sc["vw"].data_ptr(), sc["stats"].data_ptr(),
                                                                  sc["vw_rows"].data_ptr(), sc["d_vw"].data_ptr())
            a.prob_w, a.prob_b, a.reg_w, a.reg_b = (t.data_ptr() for t in hp)
            a.heads_w, a.heads_b = sc["heads_w"].data_ptr(), sc["heads_b"].data_ptr()
            a.d_heads_w, a.d_heads_b = views[HEADS_W].data_ptr(), views[HEADS_B].data_ptr()
            a.layers, a.grads = ctypes.addressof(arr), ctypes.addressof(garr)
            a.ws, a.ws_bytes = ws.data_ptr(), ws_bytes
            a.prob, a.reg, a.d_prob, a.d_reg = prob.data_ptr(), reg.data_ptr(), sc["d_prob"].data_ptr(), sc["d_reg"].data_ptr()
            a.pos, a.neg, a.targets = pos.data_ptr(), neg.data_ptr(), tgt.data_ptr()
            a.targets_stream = ts.cuda_stream if ts is not None else None
            a.alpha, a.beta, a.sigma = float(self.alpha), float(self.beta), float(self.sigma)
            a.loss_spec = spec
            a.loss_ws, a.loss_ws_bytes, a.loss5, a.g_loss = sc["loss_ws"].data_ptr(), sc["loss_ws_bytes"], loss5.data_ptr(), sc["one"].data_ptr()
            grads = self.__dict__.get("_mg_cache")
            if grads is None or grads[0] is not views:
                grads = (views, [views[n] for n, _ in self._named_params_in_flat_order()])
                self.__dict__["_mg_cache"] = grads
            out_grads = grads[1]
            # (only a plain ClipSGD's update is part of vnStep; a ClipAdamW, and a ClipSGD with a weight average attached —
            # _step_table answers False —, step after the call)
            inside = isinstance(optimizer, ClipSGD) and red is None and optimizer._step_table(plist, out_grads)
            if inside:
                a.chunks, a.n_chunks = optimizer._table.data_ptr(), optimizer._n_chunks
                a.max_norm, a.lr, a.scale_grads = optimizer.max_norm, optimizer.lr, int(optimizer.scale_grads)
                a.opt_ws, a.opt_ws_bytes, a.total_norm = optimizer._ws.data_ptr(), optimizer._ws.numel(), optimizer._norm.data_ptr()
            else:
                a.chunks, a.n_chunks, a.opt_ws, a.opt_ws_bytes, a.total_norm = None, 0, None, 0, None
            a.stream, a.side_stream = _lib.raw_stream(), self._side_stream(dev)
            a.bn_counters, a.n_bn_counters = self._counter_table(dev)
            _lib.call("vn_net_step", self._net_handle(dev), ctypes.byref(cfg), ctypes.byref(a))
            if ts is not None:
                cur = _lib.current_stream(dev)
                for t_ in targets:
                    t_.record_stream(cur)         # (allocated on the target stream, read by the loss kernels on this one)
                if self.anchor_area_threshold is not None:
                    self.last_anchor_mask.record_stream(cur)
            if red is not None:
                def waiter(bi):
                    return lambda st: _lib.call("vn_net_wait_bucket", self._net_handle(dev), bi, ctypes.c_void_p(st.cuda_stream))
                for bi in range(4):
                    red.launch_bucket(bi, wait_fn=waiter(bi))
                vfe_done = torch.cuda.Event()
                vfe_done.record()
                red.launch_bucket(4, after_event=vfe_done)
            self._ws_release(ws)
            for p_, g_ in zip(plist, out_grads):
                p_.grad = g_
            if red is not None:
                red.finish(self._named_params())
            if optimizer is not None and not inside:
                optimizer.step()
        return (prob, reg) + tuple(loss5[i] for i in range(5))

    def _named_params_in_flat_order(self):
        """(name, parameter) in _flat_params order"""
        byid = {id(p): n for n, p in self._named_params()}
        return [(byid[id(p)], p) for p in self._flat_params()]

    def _counter_table(self, dev):
        """device table of pointers to the 25 num_batches_tracked counters (vnStep.bn_counters): _tick as one launch inside
        the step call"""
        hit = self.__dict__.get("_nbt_table")
        ctrs = self.__dict__.get("_nbt")
        if ctrs is None or ctrs[0].device != dev:
            ctrs = [m.num_batches_tracked for m in self.modules()
                    if isinstance(m, (nn.BatchNorm1d, nn.BatchNorm2d, nn.BatchNorm3d))]
            self.__dict__["_nbt"] = ctrs
        key = (dev, ctrs[0].data_ptr(), ctrs[-1].data_ptr())
        if hit is None or hit[0] != key:
            if any(c.dtype != torch.int64 or c.device != dev for c in ctrs):
                raise _lib.VoxelnetHipError("num_batches_tracked: int64 counters on the step's device expected")
            tab = torch.tensor([c.data_ptr() for c in ctrs], dtype=torch.int64).to(dev)
            hit = (key, tab, len(ctrs))
            self.__dict__["_nbt_table"] = hit
        return hit[1].data_ptr(), hit[2]

    def forward(self, x, device, targets=None):
        label, voxel_features, voxel_coordinates = x[1], x[2], x[4]
        voxel_features = _parts_to(voxel_features, device)               # model.py:302-303
        voxel_coordinates = _parts_to(voxel_coordinates, device)
        # model.py:309 generates the targets AFTER the network ran; they depend on the labels only, so here their three small
        # launches (and the host-side box parsing) are issued first, on a stream of their own, and run beside the VFE /
        # first layers; the loss waits for them (529 -> 545 point-clouds/s with the targets generated inside the step)
        # (target_assign "simota" reads the maps detect() is about to produce: nothing to launch early)
        early = None
        if (targets is None and self.target_fn is None and label is not None and voxel_features and voxel_features[0].is_cuda
                and self.target_assign != "simota"):
            dev_ = voxel_features[0].device
            ts = self.__dict__.get("_tgt_stream")
            if ts is None or ts.device != dev_:
                from .voxelize import pipeline_stream
                ts = self.__dict__["_tgt_stream"] = pipeline_stream(dev_)     # (the input pipeline's stream: one queue for both)
            main = _lib.current_stream(dev_) if self.anchor_area_threshold is not None else None
            with torch.cuda.stream(ts):
                early = self._target_generator(dev_)(label)
                if main is not None:              # (right after the target generator, on its stream)
                    early = self._mask_targets(early, voxel_coordinates, main)
        prob_out, delta_out = self.detect(voxel_features, voxel_coordinates)
        if early is not None:
            cur = _lib.current_stream(prob_out.device)
            cur.wait_stream(self.__dict__["_tgt_stream"])
            for t_ in early:
                t_.record_stream(cur)         # (allocated on the target stream, read by the loss kernels on this one)
            if self.anchor_area_threshold is not None:
                self.last_anchor_mask.record_stream(cur)
            targets = early
        if targets is None:
            if self.target_fn is not None:
                targets = self.target_fn(label, self.rpn_output_shape)
            elif label is None:
                raise _lib.VoxelnetHipError("RPN3D.forward needs the batch's labels (x[1]), targets=(pos,neg,targets) or a "
                                            "target_fn")
            else:
                maps = dict(probs=prob_out.detach(), deltas=delta_out.detach()) if self.target_assign == "simota" else {}
                targets = self._target_generator(prob_out.device)(label, **maps)
                if self.anchor_area_threshold is not None:
                    targets = self._mask_targets(targets, voxel_coordinates, None)
        loss, cls_loss, reg_loss, cpos, cneg = self.loss(prob_out, delta_out, *targets)
        return prob_out, delta_out, loss, cls_loss, reg_loss, cpos, cneg
