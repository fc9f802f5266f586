"""Functional forward/backward of the middle layers + RPN (MiddleConvNet,
/root/reference/voxelnet/model.py:202-281) on channels-last rows, built from
engine.layer_forward / layer_backward.  No autograd here: model.py wraps these in
torch.autograd.Function so the reference's train loop (train.py:148-155) runs unchanged.
"""
import torch

from . import _lib
from . import engine as E
from .engine import Rows, spec2, spec3

HEADS = spec2("heads", 768, 16, 1, (1, 1), (0, 0), bn=False, relu=False)


_TABLES = {}


def layer_table(block1_stride):
    """model.py:206-254 in execution order: [(name, spec)], names = state_dict prefixes (cached: read-only)."""
    hit = _TABLES.get(block1_stride)
    if hit is None:
        hit = _TABLES[block1_stride] = _layer_table(block1_stride)
    return hit


def _layer_table(block1_stride):
    s1 = (block1_stride, block1_stride)
    t = [("middle_layer.0", spec3("middle_layer.0", 128, 64, 3, (2, 1, 1), (1, 1, 1))),
         ("middle_layer.1", spec3("middle_layer.1", 64, 64, 3, (1, 1, 1), (0, 1, 1))),
         ("middle_layer.2", spec3("middle_layer.2", 64, 64, 3, (2, 1, 1), (1, 1, 1)))]
    t += [("block1.0", spec2("block1.0", 128, 128, 3, s1, (1, 1), cin_fold=2))]
    t += [(f"block1.{i}", spec2(f"block1.{i}", 128, 128, 3, (1, 1), (1, 1))) for i in range(1, 5)]
    t += [("deconv1", spec2("deconv1", 128, 256, 3, (1, 1), (1, 1), transposed=True))]
    t += [("block2.0", spec2("block2.0", 128, 128, 3, (2, 2), (1, 1)))]
    t += [(f"block2.{i}", spec2(f"block2.{i}", 128, 128, 3, (1, 1), (1, 1))) for i in range(1, 6)]
    t += [("deconv2", spec2("deconv2", 128, 256, 2, (2, 2), (0, 0), transposed=True))]
    t += [("block3.0", spec2("block3.0", 128, 256, 3, (2, 2), (1, 1)))]
    t += [(f"block3.{i}", spec2(f"block3.{i}", 256, 256, 3, (1, 1), (1, 1))) for i in range(1, 6)]
    t += [("deconv3", spec2("deconv3", 256, 256, 4, (4, 4), (0, 0), transposed=True))]
    return t


class MiddleState:
    pass


def _dir_rows(rows, mode, what):
    """the (B*hf*wf, 768) row matrix of the concatenation (or of its gradient) for the direction head's kernels"""
    if E.is_split(mode) or rows.lo_off:
        raise ValueError(f"dir_head: {what} in a split [hi|lo] row format is not supported (DESIGN.md 1i)")
    return rows.t.view(-1, rows.t.shape[-1])


def middle_forward(dense, P, Bf, block1_stride, training, mode, sparse=None, dir_head=None, iou_head=None):
    """dense: Rows (B,D,H,W,128[hi|lo]).  P[name] = {weight,bias,gamma,beta}; Bf[name] =
    {running_mean,running_var}; P['heads'] = {weight (16,768,1,1), bias (16)}.
    sparse = (coord (K,4) int64, vw_rows (K,128) operand dtype): the occupied sites of `dense`; the first
    Conv3d then runs in its sparse form (engine.first_layer_forward_sparse) and middle_backward returns the
    (K,128) voxel gradient instead of a dense grid gradient.
    dir_head = (weight (2,768[,1,1]), bias (2)) fp32: the direction head runs on the concatenation after the
    heads, its logits (B,2,h,w) fp32 are a third output in front of the state, and the state keeps the concatenation.
    iou_head = (weight, bias) likewise: the IoU-aware confidence head, its logits the output behind the
    direction head's; with both heads on the two forwards are ONE read of the concatenation (iou_head.site_heads_forward).
    Returns prob (B,2,h,w) after sigmoid, reg (B,14,h,w) fp32 NCHW, and the saved state."""
    specs = dict(layer_table(block1_stride))
    st = MiddleState()
    st.layers = {}
    st.block1_stride = block1_stride
    st.mode = mode
    st.x3 = bool(E.X3["on"])       # (the backward runs its products as this forward did: engine._x3_as_saved)
    split = E.is_split(mode)
    dev = dense.t.device
    B = dense.B

    def run(name, x, **kw):
        a, s = E.layer_forward(specs[name], x, P[name], Bf[name], training, mode, **kw)
        st.layers[name] = s
        return a

    st.sparse = sparse if (sparse is not None and not E.is_split(mode)) else None
    if st.sparse is not None:
        x, s0 = E.first_layer_forward_sparse(specs["middle_layer.0"], dense, st.sparse[0], P["middle_layer.0"],
                                             Bf["middle_layer.0"], training, mode)
        st.layers["middle_layer.0"] = s0
    else:
        x = run("middle_layer.0", dense)
    x = run("middle_layer.1", x)
    x = run("middle_layer.2", x, bev_out=True)           # -> (B,1,H,W,128) BEV rows
    for i in range(5):
        x = run(f"block1.{i}", x)
    x1 = x
    hf, wf = specs["deconv1"].out_dims(x1.dims)[1:]
    width = 768 * (2 if split else 1)
    cat = Rows(torch.empty((B, 1, hf, wf, width), dtype=E.act_dtype_of(mode), device=dev), 768, 768 if split else 0)

    def cat_slice(off):
        return Rows(cat.t[..., off:off + 256], 256, cat.lo_off)

    run("deconv1", x1, out=cat_slice(512))               # model.py:271-273: cat([d3, d2, d1])
    for i in range(6):
        x = run(f"block2.{i}", x)
    x2 = x
    run("deconv2", x2, out=cat_slice(256))
    for i in range(6):
        x = run(f"block3.{i}", x)
    run("deconv3", x, out=cat_slice(0))
    y, s = E.layer_forward(HEADS, cat, P["heads"], None, training, mode, y_dtype=torch.float32)
    st.layers["heads"] = s
    prob = E.rows_to_nchw(Rows(y.t[..., 0:2], 2), 2, sigmoid_first_n=2)
    reg = E.rows_to_nchw(Rows(y.t[..., 2:16], 14), 2)
    st.prob = prob.detach()     # an alias, NOT the returned tensor: saving an autograd.Function's own output on its ctx is a
                                # reference cycle that only the cyclic GC frees (720 MB of dense grid per step piled up)
    st.fmap = (hf, wf)
    on = [h for h in (dir_head, iou_head) if h is not None]
    if not on:
        return prob, reg, st
    st.cat = cat
    st.dir_w = dir_head[0] if dir_head is not None else None
    st.iou_w = iou_head[0] if iou_head is not None else None
    rows = _dir_rows(cat, mode, "the concatenation")
    if len(on) == 2:
        from .iou_head import site_heads_forward
        logits = site_heads_forward(rows, [h[0] for h in on], [h[1] for h in on], B)
    else:
        from .dir_head import dir_head_forward
        logits = (dir_head_forward(rows, on[0][0], on[0][1], B),)
    return (prob, reg) + tuple(z.view(B, 2, hf, wf) for z in logits) + (st,)


def middle_backward(st, d_prob, d_reg, P, need_dx=True, on_grads=None, d_dir=None, d_iou=None):
    """-> ({name: {weight,bias,gamma,beta}}, d_dense Rows (plain f32/bf16) or None).
    on_grads(layer_name, grads): called as soon as a layer's parameter gradients exist (DDP bucketing).
    d_dir (B,2,h,w) fp32, for a forward that ran the direction head: its backward adds to the concatenation's gradient at
    the rows where d_dir is not zero, right after the heads' data gradient wrote it; G["dir_head"] = {weight, bias}.
    d_iou: the same for the IoU-aware head, after the direction head's; G["iou_head"]."""
    with E._x3_as_saved(st):
        return _middle_backward(st, d_prob, d_reg, P, need_dx, on_grads, d_dir, d_iou)


def _middle_backward(st, d_prob, d_reg, P, need_dx=True, on_grads=None, d_dir=None, d_iou=None):
    mode = st.mode
    split = E.is_split(mode)
    L = st.layers
    dev = d_prob.device
    B = d_prob.shape[0]
    hf, wf = st.fmap
    G = {}
    w16 = 32 if split else 16
    d_rows = Rows(torch.empty((B, 1, hf, wf, w16), dtype=E.act_dtype_of(mode), device=dev), 16, 16 if split else 0)
    _lib.call("vn_heads_bwd", d_prob.contiguous().data_ptr(), d_reg.contiguous().data_ptr(), st.prob.data_ptr(), B,
              hf * wf, d_rows.ptr(), E._dt(d_rows.t), w16, int(split), E.stream())
    G["heads"], d_cat = E.layer_backward(L["heads"], d_rows, P["heads"], mode)
    if on_grads is not None:
        on_grads("heads", G["heads"])
    for key, d_z, w in (("dir_head", d_dir, getattr(st, "dir_w", None)), ("iou_head", d_iou, getattr(st, "iou_w", None))):
        if d_z is None:
            continue
        from .dir_head import dir_head_backward          # (each call accumulates onto d_cat in place)
        dw, db = dir_head_backward(d_z.contiguous().float().view(B, 2, hf * wf), _dir_rows(st.cat, mode, "the concatenation"),
                                   w, _dir_rows(d_cat, mode, "the concatenation's gradient"))
        G[key] = {"weight": dw.view_as(w), "bias": db}

    def dslice(off):
        return Rows(d_cat.t[..., off:off + 256], 256)

    def back(name, da, **kw):
        g, dx = E.layer_backward(L[name], da, P[name], mode, **kw)
        G[name] = g
        if on_grads is not None:
            on_grads(name, g)
        return dx

    d = back("deconv3", dslice(0))
    for i in range(5, -1, -1):
        d = back(f"block3.{i}", d)
    d = back("deconv2", dslice(256), dx=d, dx_accumulate=True)
    for i in range(5, -1, -1):
        d = back(f"block2.{i}", d)
    d = back("deconv1", dslice(512), dx=d, dx_accumulate=True)
    for i in range(4, -1, -1):
        d = back(f"block1.{i}", d)
    d = back("middle_layer.2", d, bev_da=True)
    d = back("middle_layer.1", d)
    if st.sparse is not None:
        g0, d = E.first_layer_backward_sparse(L["middle_layer.0"], d, P["middle_layer.0"], mode, st.sparse[0],
                                              st.sparse[1])
        G["middle_layer.0"] = g0
        if on_grads is not None:
            on_grads("middle_layer.0", g0)
        return G, d          # d: (K,128) fp32 gradient of the voxel features
    d = back("middle_layer.0", d, need_dx=need_dx)
    return G, d
