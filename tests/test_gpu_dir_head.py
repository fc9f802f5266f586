"""GPU: the direction-classifier head (csrc/dir_head.hip, voxelnet_amd/dir_head.py, the dir_logits
argument of predict.BoxDecoder and RPN3D(dir_head=True)) against the float64 restatement tests/dir_ref.py on the inputs of
tests/dir_cases.py, whose guards tests/test_dir_host.py asserts on the reference alone.

Bars.
  forward   |out - ref| <= 768 * 2^-24 * sum_c |x_c w_c| + 2^-24 * (sum_c |x_c w_c| + |bias|): the worst case of an fp32 sum of 768
            products in any order, plus the one rounding of adding the bias.
  backward  listed rows of d_cat: within one unit in the last place of the stored type of the float64 result rounded to that
            type; every other row and the stride gap bit-identical.  d_w / d_bias: R * 2^-24 * sum |terms|, R listed rows.
  loss      the loss kernel's own bar: 1e-5 relative on the scalars, 1e-5 of the gradient's maximum; acc exact
            as a ratio of counts; the gradient exactly +0.0 at every non-positive.
  rectify   column 6 within 1e-6 of the NumPy decode, everything else bit-untouched.
  round trip and model: conditions, stated at the tests."""
import math
from dataclasses import replace

import numpy as np
import pytest
import torch

import dir_cases as C
import dir_ref as R
from oracle import targets as ot
from oracle import torch_ref as tr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
TDT = {"bf16": torch.bfloat16, "fp32": torch.float32}


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)          # (a writable, C-contiguous copy)


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def _vn(dtype):
    from voxelnet_amd import _lib
    return _lib.VN_BF16 if dtype == "bf16" else _lib.VN_F32


def _rows_buffer(x, dtype, stride, gap):
    """(M, 768) float32 array -> a (M, stride) device tensor of `dtype` whose first 768 columns hold x (rounded to dtype)
    and whose other columns hold `gap` (a sentinel, or random values)"""
    M = x.shape[0]
    buf = torch.empty((M, stride), dtype=torch.float32)
    buf[:, :C.C] = torch.from_numpy(np.array(x))
    if stride > C.C:
        buf[:, C.C:] = torch.as_tensor(gap, dtype=torch.float32)
    return buf.to(TDT[dtype]).to(DEV)


def _ordered(t):
    """the stored values as integers that count units in the last place across zero"""
    i = _bits(t).cpu().numpy().astype(np.int64)
    mag = i & (0x7FFF if t.dtype == torch.bfloat16 else 0x7FFFFFFF)
    return np.where(i < 0, -mag, mag)


# --------------------------------------------------------------------------------------------------------- 1. forward
@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("stride", C.STRIDES)
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("B,S", C.HEAD_SHAPES)
def test_forward_against_float64(B, S, dtype, stride, with_bias):
    from voxelnet_amd import _lib
    from voxelnet_amd.dir_head import dir_head_forward
    c = C.head_case(B, S)
    M = B * S
    rows = _rows_buffer(c["x"], dtype, stride, C.SENTINEL)
    w, bias = _dev(c["w"]), (_dev(c["bias"]) if with_bias else None)
    tail = 64
    out = torch.full((B * 2 * S + tail,), C.SENTINEL, dtype=torch.float32, device=DEV)
    _lib.call("vn_dir_head_fwd", rows.data_ptr(), _vn(dtype), stride, w.data_ptr(), bias.data_ptr() if with_bias else None, B, S,
              out.data_ptr(), _lib.raw_stream())
    got = out[:B * 2 * S].view(B, 2, S).cpu().numpy().astype(np.float64)
    assert bool((out[B * 2 * S:] == C.SENTINEL).all())                                  # nothing behind the logits is written
    assert bool((rows[:, C.C:] == C.SENTINEL).all())
    ref, mag = R.head_forward(rows[:, :C.C].cpu().double().numpy(), c["w"], c["bias"] if with_bias else None)
    ref, mag = ref.reshape(B, S, 2).transpose(0, 2, 1), mag.reshape(B, S, 2).transpose(0, 2, 1)
    bound = C.C * U * mag + U * (mag + (np.abs(c["bias"]).astype(np.float64)[None, :, None] if with_bias else 0.0))
    err = np.abs(got - ref)
    print(f"forward {B}x{S} {dtype} stride {stride} bias {with_bias}: max err {err.max():.3e}, max err / bound {(err / bound).max():.3e}")
    assert (err <= bound).all(), float((err / bound).max())
    # the wrapper: the same launch on a view of the rows
    via = dir_head_forward(rows[:, :C.C], w, bias, B)
    assert via.shape == (B, 2, S) and torch.equal(_bits(via), _bits(out[:B * 2 * S].view(B, 2, S)))


# -------------------------------------------------------------------------------------------------------- 2. backward
def _backward(g, rows, dtype, w, d_cat, ddtype, dstride, B, S, ws_bytes=None):
    from voxelnet_amd import _lib
    gl = _dev(g.reshape(B, S, 2).transpose(0, 2, 1))                                  # (B, 2, S)
    need = _lib.load().vn_dir_head_bwd_workspace_bytes(B, S)
    nbytes = need if ws_bytes is None else ws_bytes
    ws = torch.empty(max(need, 1), dtype=torch.uint8, device=DEV)
    d_w = torch.full((2, C.C), C.SENTINEL, dtype=torch.float32, device=DEV)
    d_b = torch.full((2,), C.SENTINEL, dtype=torch.float32, device=DEV)
    _lib.call("vn_dir_head_bwd", gl.data_ptr(), rows.data_ptr(), _vn(dtype), rows.stride(0), w.data_ptr(), B, S, d_cat.data_ptr(),
              _vn(ddtype), dstride, d_w.data_ptr(), d_b.data_ptr(), ws.data_ptr(), nbytes, _lib.raw_stream())
    return d_w, d_b


@pytest.mark.parametrize("pattern", C.PATTERNS)
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("B,S", C.HEAD_SHAPES)
def test_backward_against_float64(B, S, dtype, pattern):
    c = C.head_case(B, S)
    M, dstride = B * S, 1024
    g, listed = C.grad_pattern(pattern, B, S)
    rows = _rows_buffer(c["x"], dtype, C.C, 0.0)
    w = _dev(c["w"])
    gap = np.random.default_rng(5).standard_normal((M, dstride - C.C)).astype(np.float32)
    before = _rows_buffer(c["d_cat"], dtype, dstride, gap)
    d1, d2 = before.clone(), before.clone()
    dw1, db1 = _backward(g, rows, dtype, w, d1, dtype, dstride, B, S)
    dw2, db2 = _backward(g, rows, dtype, w, d2, dtype, dstride, B, S)
    for a, b in ((d1, d2), (dw1, dw2), (db1, db2)):                                     # two calls are bit-equal
        assert torch.equal(_bits(a), _bits(b))
    skipped = np.ones(M, dtype=bool)
    skipped[listed] = False
    sk = torch.from_numpy(skipped).to(DEV)
    assert torch.equal(_bits(d1[sk]), _bits(before[sk]))                                # rows without a gradient: not touched
    assert torch.equal(_bits(d1[:, C.C:]), _bits(before[:, C.C:]))                      # nor the stride gap of any row
    x64, d64 = rows.cpu().double().numpy(), before[:, :C.C].cpu().double().numpy()
    ref_d, ref_w, ref_b, mag_w, mag_b = R.head_backward(g[listed], x64[listed], c["w"], d64[listed])
    R_ = len(listed)
    if R_:
        want = torch.from_numpy(ref_d).to(TDT[dtype])                                  # the float64 result rounded to the stored type
        ulps = np.abs(_ordered(d1[torch.as_tensor(listed, device=DEV)][:, :C.C]) - _ordered(want))
        print(f"backward {B}x{S} {dtype} {pattern}: {R_} rows, d_cat max ulps {ulps.max()}")
        assert ulps.max() <= 1
        assert not torch.equal(_bits(d1[listed[0], :C.C]), _bits(before[listed[0], :C.C]))
    else:
        assert torch.equal(_bits(d1), _bits(before))
        assert not dw1.any() and not db1.any()                                          # exactly zero
    ew, eb = np.abs(dw1.cpu().double().numpy() - ref_w), np.abs(db1.cpu().double().numpy() - ref_b)
    print(f"backward {B}x{S} {dtype} {pattern}: d_w max err {ew.max():.3e} (bound {np.max(R_ * U * mag_w):.3e}), d_bias {eb.max():.3e}")
    assert (ew <= R_ * U * mag_w).all() and (eb <= R_ * U * mag_b).all()


def test_backward_mixed_dtypes_and_short_workspace():
    from voxelnet_amd import _lib
    from voxelnet_amd.dir_head import dir_head_backward
    B, S = 2, 70
    c = C.head_case(B, S)
    g, listed = C.grad_pattern("spread", B, S)
    w = _dev(c["w"])
    # bf16 rows with an fp32 gradient buffer, through the wrapper
    rows = _rows_buffer(c["x"], "bf16", C.C, 0.0)
    before = _rows_buffer(c["d_cat"], "fp32", C.C, 0.0)
    d = before.clone()
    dw, db = dir_head_backward(_dev(g.reshape(B, S, 2).transpose(0, 2, 1)), rows, w, d)
    ref_d, ref_w, ref_b, mag_w, mag_b = R.head_backward(g[listed], rows.cpu().double().numpy()[listed], c["w"],
                                                        before.cpu().double().numpy()[listed])
    assert np.abs(_ordered(d[torch.as_tensor(listed, device=DEV)]) - _ordered(torch.from_numpy(ref_d).float())).max() <= 1
    assert (np.abs(dw.cpu().double().numpy() - ref_w) <= len(listed) * U * mag_w).all()
    assert (np.abs(db.cpu().double().numpy() - ref_b) <= len(listed) * U * mag_b).all()
    need = _lib.load().vn_dir_head_bwd_workspace_bytes(B, S)
    with pytest.raises(_lib.VoxelnetHipError, match="workspace too small"):
        _backward(g, rows, "bf16", w, d, "fp32", C.C, B, S, ws_bytes=need - 1)
    with pytest.raises(_lib.VoxelnetHipError, match="invalid argument"):          # a split row format is refused
        _lib.call("vn_dir_head_bwd", d.data_ptr(), rows.data_ptr(), _lib.VN_F32X3S, C.C, w.data_ptr(), B, S, d.data_ptr(), _lib.VN_F32,
                  C.C, dw.data_ptr(), db.data_ptr(), d.data_ptr(), need, _lib.raw_stream())


# ------------------------------------------------------------------------------------------------------------ 3. loss
def _loss_call(c, off, with_grad):
    from voxelnet_amd import _lib
    B, h, w = c["pos"].shape[:3]
    z, pos, tg, an = _dev(c["logits"]), _dev(c["pos"]), _dev(c["targets"]), _dev(c["anchors"].reshape(-1, 7))
    nbytes = _lib.load().vn_rpn_dir_loss_workspace_bytes(B, h, w)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    out = torch.full((2,), C.SENTINEL, dtype=torch.float32, device=DEV)
    d = torch.full_like(z, C.SENTINEL) if with_grad else None
    _lib.call("vn_rpn_dir_loss", z.data_ptr(), pos.data_ptr(), tg.data_ptr(), an.data_ptr(), B, h, w, float(off), ws.data_ptr(), nbytes,
              out.data_ptr(), d.data_ptr() if with_grad else None, _lib.raw_stream())
    return out, d


def _check_loss(c, shape, off):
    """the raw call, with and without the gradient, against dir_ref at the loss' bars -> (out2, d_logits, the non-positives)"""
    L, acc, grad, (hits, n) = R.loss(c["logits"], c["pos"], c["targets"], c["anchors"], off)
    out, d = _loss_call(c, off, True)
    fwd, _ = _loss_call(c, off, False)
    assert torch.equal(_bits(out), _bits(fwd))                                          # d_logits = NULL: the same scalars
    got = out.cpu().numpy()
    eg = np.abs(d.cpu().double().numpy() - grad).max()
    print(f"loss {shape} offset {off:.4f}: L {got[0]:.7f} vs {L:.7f} (rel {abs(got[0] - L) / L:.2e}), acc {got[1]:.6f} = {hits}/{n}, "
          f"gradient err / max {eg / np.abs(grad).max():.2e}")
    assert abs(float(got[0]) - L) <= 1e-5 * abs(L)
    assert got[1] == np.float32(hits / max(1, n)) and 0 < hits < n
    assert eg <= 1e-5 * np.abs(grad).max()
    off_pos = _dev(R.site_layout(c["pos"]) == 0)
    assert bool((_bits(d)[off_pos] == 0).all())                                         # exactly +0.0 at every non-positive
    assert bool((d[~off_pos] != 0).all())
    return out, d, off_pos


@pytest.mark.parametrize("off", C.OFFSETS, ids=["pi4", "zero"])
@pytest.mark.parametrize("shape", list(C.SEAM_CASES), ids=lambda s: "x".join(str(v) for v in s))
def test_loss_seams_of_the_site_term_scaffold(shape, off):
    """the two loops of csrc/rpn_common.h's scaffold that no LOSS_SHAPES entry reaches (dir_cases.SEAM_CASES, guarded on the
    CPU by tests/test_dir_host.py): k_pos_norm's second sweep over a sample, and k_site_term_finalize's second slab row per
    thread with a workgroup that straddles two samples.  test_loss_against_dir_ref's comparisons and bars."""
    _check_loss(C.seam_case(shape), shape, off)


@pytest.mark.parametrize("off", C.OFFSETS, ids=["pi4", "zero"])
@pytest.mark.parametrize("shape", C.LOSS_SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_loss_against_dir_ref(shape, off):
    from voxelnet_amd import _lib
    from voxelnet_amd.dir_head import rpn_dir_loss
    c = C.loss_case(shape)
    out, d, off_pos = _check_loss(c, shape, off)
    # the autograd Function: the same scalars; the gradient scaled by the upstream one; acc carries none
    z = _dev(c["logits"]).requires_grad_(True)
    an = _dev(c["anchors"])
    loss, a = rpn_dir_loss(z, _dev(c["pos"]), _dev(c["targets"]), an, off)
    assert torch.equal(_bits(torch.stack([loss.detach(), a])), _bits(out)) and not a.requires_grad
    (0.2 * loss).backward()
    assert torch.allclose(z.grad, 0.2 * d, rtol=1e-6, atol=0) and bool((_bits(z.grad)[off_pos] == 0).all())
    with pytest.raises(_lib.VoxelnetHipError, match="invalid argument"):
        _loss_call(c, float("nan"), True)


# --------------------------------------------------------------------------------------------------------- 4. rectify
def test_rectify_yaw_against_the_numpy_decode():
    from voxelnet_amd import _lib
    from voxelnet_amd.dir_head import rectify_yaw
    c = C.rectify_case()
    B, K = c["idx"].shape
    S = c["S"]
    tail = 16
    for off in C.OFFSETS:
        buf = torch.full((B * K * 7 + tail,), C.SENTINEL, dtype=torch.float32, device=DEV)
        buf[:B * K * 7] = _dev(c["boxes"]).reshape(-1)
        boxes = buf[:B * K * 7].view(B, K, 7)
        before = boxes.clone()
        got = rectify_yaw(boxes, _dev(c["idx"]), _dev(c["counts"]), _dev(c["logits"]), 2 * S, off)
        assert got is boxes and bool((buf[B * K * 7:] == C.SENTINEL).all())
        g, b0 = boxes.cpu().numpy(), before.cpu().numpy()
        assert np.array_equal(g[..., :6].view(np.uint32), b0[..., :6].view(np.uint32))
        worst = 0.0
        for b in range(B):
            n = min(int(c["counts"][b]), K)
            idx = c["idx"][b, :n].astype(np.int64)
            want = R.rectify(b0[b, :n, 6], c["logits"][b, idx & 1, idx >> 1], off)
            if n:
                worst = max(worst, float(np.abs(g[b, :n, 6] - want).max()))
                assert off <= want.min() and want.max() < off + 2 * np.pi
            assert np.array_equal(g[b, n:, 6].view(np.uint32), b0[b, n:, 6].view(np.uint32))          # rows past the count
        print(f"rectify offset {off:.4f}: max |yaw - reference| {worst:.3e}")
        assert worst <= 1e-6
    z0 = c["logits"][0, c["idx"][0, 0] & 1, c["idx"][0, 0] >> 1]
    assert z0 == 0.0 and g[0, 0, 6] < C.OFFSETS[-1] + np.pi                             # a logit of exactly 0: bin 0
    with pytest.raises(_lib.VoxelnetHipError, match="invalid argument"):
        _lib.call("vn_boxes_rectify_yaw", boxes.data_ptr(), _dev(c["idx"]).data_ptr(), _dev(c["counts"]).data_ptr(),
                  _dev(c["logits"]).data_ptr(), B, K, 2 * S - 1, 0.0, _lib.raw_stream())
    with pytest.raises(ValueError):
        rectify_yaw(boxes, _dev(c["idx"]), _dev(c["counts"]), _dev(c["logits"]), 2 * S - 1)


# ------------------------------------------------------------------------------------------------------ 5. round trip
def _perfect_maps(pos, targets):
    """tests/test_gpu_detect_site.py's, restated: prob (B,2,h,w) = 0.05 + pos * (0.9 + distinct multiples of 2^-22), delta
    (B,14,h,w) = targets — the maps of a network that has fitted the loss's targets exactly; and the positives' rank"""
    p = pos.reshape(-1)
    rank = torch.cumsum(p, 0) * p
    assert float(rank.max()) < 2 ** 17
    prob = (0.05 + p * (0.9 + rank * 2.0 ** -22)).reshape(pos.shape).permute(0, 3, 1, 2).contiguous()
    return prob, targets.permute(0, 3, 1, 2).contiguous(), rank.reshape(pos.shape)


@pytest.mark.parametrize("kind", ["standup", "rotated"])
def test_round_trip_heading_survives_the_sine_loss(kind):
    """The test that fails without the feature.  Maps of a network that has minimised the sine loss: the regression
    channels equal the targets, except that the yaw channel is off by pi at every second positive — smooth_L1(sin) cannot
    tell — and the direction logits name the bin of the matched box's yaw.  Decoded with the logits, every detection
    faces the way its ground truth does and AOS equals the `bbox` AP; without them the same boxes come back with
    headings wrong by pi and AOS falls at least 0.2 below the AP."""
    from voxelnet_amd.dir_head import rpn_dir_loss
    from voxelnet_amd.evaluate import KittiDetectionEvaluator
    from voxelnet_amd.predict import TRAINED_DECODE, BoxDecoder
    from voxelnet_amd.targets import TargetGenerator
    anchors = C.round_trip_anchors()
    labels, gt = C.round_trip_frames(anchors)
    gen = TargetGenerator("Car", DEV, anchors=anchors, assign=kind, keep_heading=True)
    pos, neg, targets = gen(labels)
    assert [int(v) for v in pos.reshape(3, -1).sum(dim=1).tolist()][2] == 0
    prob, delta, rank = _perfect_maps(pos, targets)
    flip = ((rank % 2) == 1) & (pos != 0)                                               # every second positive: the 1st, 3rd, ...
    off_by_pi = targets.clone()
    off_by_pi[..., 6] += math.pi * flip[..., 0]
    off_by_pi[..., 13] += math.pi * flip[..., 1]
    delta = off_by_pi.permute(0, 3, 1, 2).contiguous()
    th = R.theta_gt(targets.cpu().numpy(), anchors)
    pm = pos.cpu().numpy() != 0
    assert R.edge_gap(th)[pm].min() > R.EDGE                                            # the guard, on the reference
    dirl = _dev(np.where(R.dir_bin(th) == 1, 4.0, -4.0).astype(np.float32)).permute(0, 3, 1, 2).contiguous()      # (B,2,h,w)
    dec = BoxDecoder("Car", DEV, anchors=anchors)
    kw = dict(TRAINED_DECODE, score_thres=0.5, top_k=20)
    with_head = dec.decode_device(prob, delta, **kw, dir_logits=dirl)
    without = dec.decode_device(prob, delta, **kw)
    assert with_head[2].tolist() == without[2].tolist() == [4, 2, 0]                    # one detection per ground truth
    assert torch.equal(_bits(with_head[0][..., :6]), _bits(without[0][..., :6])) and torch.equal(_bits(with_head[1]), _bits(without[1]))
    right, wrong = [], []
    for b, g in enumerate(gt):
        taken = set()
        for k in range(len(g)):
            bw, bo = with_head[0][b, k].cpu().numpy().astype(np.float64), without[0][b, k].cpu().numpy().astype(np.float64)
            j = int(np.argmin(np.hypot(g[:, 0] - bw[0], g[:, 1] - bw[1])))
            assert j not in taken and np.hypot(g[j, 0] - bw[0], g[j, 1] - bw[1]) < 0.05
            taken.add(j)
            right.append(math.cos(bw[6] - g[j, 6]))
            wrong.append(math.cos(bo[6] - g[j, 6]))
    print(f"{kind}: cos(yaw_det - yaw_gt) with the head {[f'{c:.9f}' for c in right]}, without {[f'{c:.6f}' for c in wrong]}")
    assert len(right) == 6 and min(right) >= 1 - 1e-6
    assert sum(c <= -1 + 1e-6 for c in wrong) >= 2
    res = {}
    for name, det in (("with", with_head), ("without", without)):
        ev = KittiDetectionEvaluator("Car", DEV, top_k=20)
        ev.update(*det, labels)
        res[name] = ev.compute()
        print(f"{kind} {name} the head: bbox {res[name]['bbox']}, aos {res[name]['aos']}")
    assert res["with"]["n_gt"]["all"] == 6 and res["with"]["bbox"]["all"] == 1.0
    for d, ap in res["with"]["bbox"].items():
        assert res["with"]["aos"][d] >= ap - 1e-6, d
        assert res["without"]["bbox"][d] == ap and res["without"]["aos"][d] <= ap - 0.2, d
    _, acc = rpn_dir_loss(dirl, pos, targets, gen._anchors_dev)
    assert float(acc) == 1.0
    with pytest.raises(ValueError):
        dec.decode_device(prob, delta, **dict(kw, layout="flat"), dir_logits=dirl)
    cb, _, _, cc = dec.candidates_device(prob, delta, 0.5, 64, layout="site", dir_logits=dirl)
    assert int(cc.sum()) >= 6
    for b in range(3):                                                                  # the candidates' yaws are rectified too
        y = cb[b, :int(cc[b]), 6]
        assert bool(((y >= math.pi / 4 - 1e-6) & (y < math.pi / 4 + 2 * math.pi + 1e-6)).all())


# ------------------------------------------------------------------------------------------------------------ 6. model
ANCHORS_TINY = np.ascontiguousarray(ot.generate_anchors("Car")[:8, :12])


def _tiny(golden):
    g, t = golden("middle_tiny_car"), golden("rpn3d_tiny")
    lens = [int(x) for x in g["feat_lens"]]
    feats = list(torch.split(torch.from_numpy(g["features"]), lens))
    coords = list(torch.split(torch.from_numpy(g["coords"]), lens))
    targets = tuple(np.ascontiguousarray(t[k], dtype=np.float32) for k in ("pos", "neg", "targets"))
    batch = (["000000", "000001"], None, [f.to(DEV) for f in feats], None, [c.to(DEV) for c in coords], None, None)
    return feats, coords, targets, batch


def _tiny_model(mode, native=True, **kw):
    from voxelnet_amd import model as M
    from voxelnet_amd.targets import TargetGenerator
    M.set_precision(mode)
    torch.manual_seed(7)
    m = M.RPN3D("Car", **kw)
    res = m.load_state_dict(tr.make_state_dict("Car"), strict=False)
    assert all("dir_conv" in k for k in res.missing_keys) and not res.unexpected_keys
    m.feature_net._grid = replace(m.feature_net._grid, H=16, W=24)
    m.native_executor = native
    m = m.to(DEV).train()
    m.__dict__["_targets"] = TargetGenerator("Car", DEV, anchors=ANCHORS_TINY, keep_heading=bool(kw.get("dir_head")))
    return m


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_model_zero_weight_head_changes_nothing(golden, mode):
    """(b): a head whose loss weight is 0 sends a gradient of zeros, which the backward skips — maps, the five scalars
    and all 104 gradients are those of the per-layer orchestration without the head, bit for bit"""
    from voxelnet_amd import model as M
    _, _, targets, batch = _tiny(golden)
    try:
        a = _tiny_model(mode, native=False)
        assert not a._native_ok(mode)
        out_a = a(batch, DEV, targets=targets)
        out_a[2].backward()
        h = _tiny_model(mode, dir_head=True, dir_weight=0.0)
        out_h = h(batch, DEV, targets=targets)
        out_h[2].backward()
        torch.cuda.synchronize()
    finally:
        M.set_precision("bf16")
    assert len(out_a) == len(out_h) == 7
    for i, (x, y) in enumerate(zip(out_a, out_h)):
        assert torch.isfinite(x).all() and torch.equal(_bits(x.detach().float()), _bits(y.detach().float())), (mode, i)
    ga, gh = dict(a.named_parameters()), dict(h.named_parameters())
    assert len(ga) == 104 and len(gh) == 106
    for k in ga:
        assert ga[k].grad is not None and torch.equal(_bits(ga[k].grad), _bits(gh[k].grad)), (mode, k)
    for k in set(gh) - set(ga):
        assert gh[k].grad is not None and not gh[k].grad.any(), k                        # the all-zero pattern: exactly 0
    assert h.last_dir_logits.shape == (2, 2, 8, 12) and h.last_dir is not None and a.last_dir is None


def test_model_head_against_the_float64_oracle(golden):
    """(c): fp32, dir_weight 0.2.  The reference is the CPU oracle's float64 train-mode forward with its taps: the concat
    is cat([deconv3, deconv2, deconv1]), a float64 1x1 convolution gives the logits, dir_ref's loss joins the oracle's
    rpn_loss, autograd runs through the trunk.  Logits at the fp32 map bar (1e-3 relative).  Gradients at the bars
    tests/test_gpu_model.py::test_detect_fwd_bwd_fp32 applies on this fixture: relative L2 < 5e-2 for parameters under the
    ReLU stack (its line 126: deconv3's and block1.0's weights), max error < 1e-3 of the maximum for parameters with no
    ReLU behind them (its line 128, there the heads: here dir_conv's weight and bias)."""
    import torch.nn.functional as F
    from voxelnet_amd import model as M
    feats, coords, targets, batch = _tiny(golden)
    pos_n, neg_n, tgt_n = targets
    assert R.edge_gap(R.theta_gt(tgt_n, ANCHORS_TINY))[pos_n != 0].min() > R.EDGE         # the guard, on the reference
    try:
        h = _tiny_model("fp32", dir_head=True, dir_weight=0.2)
        out = h(batch, DEV, targets=targets)
        out[2].backward()
        torch.cuda.synchronize()
    finally:
        M.set_precision("bf16")
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in tr.make_state_dict("Car").items()}
    dk = ("middle_rpn.dir_conv.conv.weight", "middle_rpn.dir_conv.conv.bias")
    for k in dk:
        sd[k] = dict(h.named_parameters())[k].detach().cpu().double()
    keys = tr.param_keys(sd) + [k for k in dk if k not in tr.param_keys(sd)]
    leaves = {k: sd[k].detach().clone().requires_grad_(True) for k in keys}
    work = dict(sd)
    work.update(leaves)
    taps = {}
    prob, reg = tr.middle_rpn(tr.feature_net([f.double() for f in feats], coords, work, (10, 16, 24), True), work, "Car", True, taps=taps)
    cat = torch.cat([taps["deconv3"], taps["deconv2"], taps["deconv1"]], dim=1)
    logits = F.conv2d(cat, leaves[dk[0]], leaves[dk[1]])
    pos, neg, tgt = (torch.from_numpy(a).double() for a in targets)
    l_dir, _, _ = R.loss_torch(logits.reshape(2, 2, -1), pos_n, tgt_n, ANCHORS_TINY)
    ref_out = tr.rpn_loss(prob, reg, pos, neg, tgt)
    (ref_out[0] + 0.2 * l_dir).backward()
    l_dir, ref_out = l_dir.detach(), [o.detach() for o in ref_out]
    ez = float((h.last_dir_logits.detach().cpu().double() - logits.detach()).abs().max() / logits.detach().abs().max())
    print(f"dir logits vs the float64 oracle: {ez:.2e}; L_dir {float(h.last_dir[0]):.6f} vs {float(l_dir):.6f}, acc {float(h.last_dir[1]):.4f}")
    assert ez < 1e-3
    assert abs(float(h.last_dir[0]) - float(l_dir)) <= 2e-3 * abs(float(l_dir))           # (test_rpn3d_forward_loss's bar on the scalars)
    np.testing.assert_allclose(float(out[2].detach()), float(ref_out[0] + 0.2 * l_dir), rtol=2e-3)
    np.testing.assert_allclose(float(out[3].detach()), float(ref_out[1] + 0.2 * l_dir), rtol=2e-3)
    got = dict(h.named_parameters())
    for k in dk + ("middle_rpn.deconv3.deconv.weight", "middle_rpn.block1.0.conv.weight"):
        r = leaves[k].grad.numpy()
        q = got[k].grad.detach().cpu().double().numpy()
        e, l2 = float(np.abs(q - r).max() / np.abs(r).max()), float(np.linalg.norm(q - r) / np.linalg.norm(r))
        print(f"{k}: max err {e:.2e}, relative L2 {l2:.2e}")
        assert np.linalg.norm(r) > 0
        if k in dk:
            assert e < 1e-3, (k, e)
        else:
            assert l2 < 5e-2, (k, l2)


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_model_train_step_equals_separate_calls_with_the_head(golden, mode):
    """(d): with the head on, train_step takes its separate-calls branch (the head is outside the native executor) and
    equals forward + backward as separate module calls bit for bit; the head's loss is part of the result"""
    from voxelnet_amd import model as M
    _, _, targets, batch = _tiny(golden)
    try:
        a = _tiny_model(mode, dir_head=True)
        assert not a._step_fused_ok(mode, None) and not a._native_ok(mode)
        out_a = a.train_step(batch, DEV, None, targets=targets)
        b = _tiny_model(mode, dir_head=True)
        out_b = b(batch, DEV, targets=targets)
        out_b[2].backward()
        c = _tiny_model(mode, native=False)
        out_c = c(batch, DEV, targets=targets)
        torch.cuda.synchronize()
    finally:
        M.set_precision("bf16")
    for i, (x, y) in enumerate(zip(out_a, out_b)):
        assert torch.isfinite(x).all() and torch.equal(x, y), (mode, i)
    ga, gb = dict(a.named_parameters()), dict(b.named_parameters())
    assert len(ga) == 106
    for k in ga:
        assert ga[k].grad is not None and torch.isfinite(ga[k].grad).all() and torch.equal(ga[k].grad, gb[k].grad), (mode, k)
    assert ga["middle_rpn.dir_conv.conv.weight"].grad.abs().max() > 0
    l_dir = float(a.last_dir[0])
    assert l_dir > 0 and float(out_a[2]) == pytest.approx(float(out_c[2]) + 0.2 * l_dir, rel=1e-5)
    assert float(out_a[3]) == pytest.approx(float(out_c[3]) + 0.2 * l_dir, rel=1e-5) and float(out_a[4]) == float(out_c[4])


def test_model_evaluate_reaches_rectify_yaw(golden, monkeypatch):
    """(e): evaluate(decode=TRAINED_DECODE) and predict(decode=) hand the head's logits to the decoder, whose composed tail
    calls vn_boxes_rectify_yaw; a decode that does not read the maps by site is refused; (f): fp32x3 and a reducer too"""
    from voxelnet_amd import _lib, synth
    from voxelnet_amd import model as M
    from voxelnet_amd.evaluate import DetectionEvaluator
    from voxelnet_amd.predict import EVAL_DECODE, TRAINED_DECODE, BoxDecoder
    _, _, targets, batch = _tiny(golden)
    labels = [synth.synth_labels("Car", 3, 40 + b) for b in range(2)]
    batches = [(batch[0], labels) + batch[2:]]
    names, real = [], _lib.call

    def recording(name, *args):
        names.append(name)
        return real(name, *args)
    try:
        h = _tiny_model("bf16", dir_head=True)
        dec = BoxDecoder("Car", DEV, anchors=ANCHORS_TINY)
        ev = DetectionEvaluator("Car", DEV)
        decode = dict(TRAINED_DECODE, score_thres=0.0)
        monkeypatch.setattr(_lib, "call", recording)
        assert h.evaluate(batches, DEV, evaluator=ev, decoder=dec, decode=decode) is ev
        monkeypatch.setattr(_lib, "call", real)
        for want in ("vn_dir_head_fwd", "vn_rpn_select_decode_layout", "vn_boxes_rectify_yaw", "vn_box_nms"):
            assert want in names, want
        assert names.index("vn_rpn_select_decode_layout") < names.index("vn_boxes_rectify_yaw") < names.index("vn_box_nms")
        assert "vn_net_forward" not in names and h.training                              # the per-layer path; the mode is restored
        assert ev.compute()["n_det"] > 0
        with pytest.raises(ValueError, match="site"):
            h.evaluate(batches, DEV, decoder=dec, decode=EVAL_DECODE)
        h.__dict__["_decoder"] = dec
        with torch.no_grad():
            prob, delta = h.detect(batch[2], batch[4])
        names.clear()
        monkeypatch.setattr(_lib, "call", recording)
        tag, rows = h.predict((batch[0],), prob, delta, decode=dict(decode, top_k=20))
        monkeypatch.setattr(_lib, "call", real)
        assert "vn_boxes_rectify_yaw" in names and len(rows) == 2 and sum(len(r) for r in rows) > 0
        yaws = np.concatenate([r[:, 7].astype(np.float64) for r in rows])
        assert (yaws >= math.pi / 4 - 1e-6).all() and (yaws < math.pi / 4 + 2 * math.pi + 1e-6).all()
        with pytest.raises(ValueError, match="site"):
            h.predict((batch[0],), prob, delta)
        # (f)
        h.grad_reducer = object()
        with pytest.raises(ValueError, match="grad_reducer"):
            h(batch, DEV, targets=targets)
        h.grad_reducer = None
        M.set_precision("fp32x3")
        with pytest.raises(ValueError, match="fp32x3"):
            h(batch, DEV, targets=targets)
        with pytest.raises(ValueError, match="fp32x3"):
            h.middle_rpn(torch.zeros(1, 10, 16, 24, 128, device=DEV))
    finally:
        M.set_precision("bf16")


def test_model_checkpoints_with_and_without_the_head(golden):
    """(a) and (g) on the device: a default model carries no trace of the head and still takes the native executor; a
    state_dict with the head round-trips; a head-less checkpoint loads with strict=False, the two new keys missing"""
    from voxelnet_amd import model as M
    _, _, targets, batch = _tiny(golden)
    try:
        a, d = _tiny_model("bf16"), _tiny_model("bf16", dir_head=False)
        assert list(a.state_dict()) == list(d.state_dict()) and not any("dir_conv" in k for k in a.state_dict())
        assert a._native_ok("bf16") and a._step_fused_ok("bf16", None)
        h = _tiny_model("bf16", dir_head=True)
        h2 = _tiny_model("bf16", dir_head=True)
        with torch.no_grad():
            h2.middle_rpn.dir_conv.conv.weight.add_(1.0)
        assert h2.load_state_dict(h.state_dict()).missing_keys == []
        res = h2.load_state_dict(a.state_dict(), strict=False)
        assert sorted(res.missing_keys) == ["middle_rpn.dir_conv.conv.bias", "middle_rpn.dir_conv.conv.weight"]
        with torch.no_grad():
            pa, _ = a.detect(batch[2], batch[4])
            ph, _ = h2.detect(batch[2], batch[4])
        assert a.last_dir_logits is None and h2.last_dir_logits.shape == (2, 2, 8, 12)
        assert torch.isfinite(ph).all() and pa.shape == ph.shape
    finally:
        M.set_precision("bf16")
