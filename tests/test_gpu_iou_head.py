"""GPU: the IoU-aware confidence head (csrc/iou_head.hip, voxelnet_amd/iou_head.py, the iou_logits
argument of predict.BoxDecoder and RPN3D(iou_head=True)) against the float64 restatement tests/iou_head_ref.py on the inputs
of tests/iou_head_cases.py, whose guards tests/test_iou_head_host.py asserts on the reference alone.

Bars.
  loss      the project's own for its float64 site terms: 1e-5 relative on the two scalars, 1e-5 of the
            gradient's maximum; the gradient exactly +0.0 at every non-positive.  Measured here: see DESIGN.md 1l.
  target    1e-6 relative against vn_box_iou_rotated on boxes decoded in NumPy (test_gpu_iou_loss's bar for the same pair of
            computations), +0.0 elsewhere.
  rectify   within one unit in the last place of fp32 of NumPy's float64 pow rounded to fp32 (device and host pow / exp may
            differ in the last place of a double, which can move the fp32 rounding by one step); alpha = 0 by bits.
  fused     by bits against vn_dir_head_fwd.
  round trip and model: conditions, stated at the tests."""
import math
from dataclasses import replace

import numpy as np
import pytest
import torch

import dir_cases as DC
import iou_head_cases as C
import iou_head_ref as R
from oracle import torch_ref as tr
from test_gpu_dir_head import ANCHORS_TINY, _bits, _ordered, _rows_buffer, _tiny, _vn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TAIL = 64
_ids3 = lambda s: "x".join(str(v) for v in s[:3])          # noqa: E731


def _dev(a):
    a = a.numpy() if torch.is_tensor(a) else a
    return torch.from_numpy(np.array(a, order="C")).to(DEV)


def _guarded(n):
    """n float32 elements followed by TAIL sentinels -> (the whole buffer, the first n)"""
    buf = torch.full((n + TAIL,), C.SENTINEL, dtype=torch.float32, device=DEV)
    return buf, buf[:n]


def _raw_loss(case, metric, with_grad=True, with_target=True, ws_bytes=None):
    """vn_rpn_iou_head_loss on a workspace of 0xA5 bytes, sentinels behind every output -> (out2, d_logits, iou_target)"""
    from voxelnet_amd import _lib
    from voxelnet_amd.iou_loss import METRICS
    z, delta, pos, tgt, an = (_dev(v) for v in case)
    B, H, W, _ = pos.shape
    need = _lib.load().vn_rpn_iou_head_loss_workspace_bytes(B, H, W)
    ws = torch.full((need + TAIL,), 0xA5, dtype=torch.uint8, device=DEV)
    n = B * 2 * H * W
    ob, out = _guarded(2)
    db, d = _guarded(n)
    tb, t = _guarded(n)
    _lib.call("vn_rpn_iou_head_loss", z.data_ptr(), delta.data_ptr(), pos.data_ptr(), tgt.data_ptr(), an.data_ptr(), B, H, W,
              METRICS.get(metric, metric), ws.data_ptr(), need if ws_bytes is None else ws_bytes, out.data_ptr(),
              d.data_ptr() if with_grad else None, t.data_ptr() if with_target else None, _lib.raw_stream())
    for b_, used in ((ob, True), (db, with_grad), (tb, with_target)):
        assert bool((b_[-TAIL:] == C.SENTINEL).all())
        if not used:
            assert bool((b_ == C.SENTINEL).all())
    assert bool((ws[need:] == 0xA5).all())
    return out, d.view(B, 2, H * W), t.view(B, 2, H * W)


def _check_loss(case, shape, metric, n_pairs_min):
    L, mae, grad, t_ref, pairs = R.loss(case[0].numpy(), *case[1:], metric)
    assert len(pairs) >= n_pairs_min and all(p[1] > 0.0 for p in pairs)               # no pair is silently trivial
    out, d, t = _raw_loss(case, metric)
    got = out.cpu().double().numpy()
    eL, eM = abs(got[0] - L) / abs(L), abs(got[1] - mae) / abs(mae)
    eg = np.abs(d.cpu().double().numpy() - grad).max() / np.abs(grad).max()
    et = np.abs(t.cpu().double().numpy() - t_ref).max()
    print(f"iou head loss {shape[:3]} {metric}: L {got[0]:.7f} vs {L:.7f} (rel {eL:.2e}), mae {got[1]:.7f} vs {mae:.7f} (rel {eM:.2e}), "
          f"gradient err / max {eg:.2e}, target err {et:.2e}")
    assert eL <= 1e-5 and eM <= 1e-5 and eg <= 1e-5
    assert et <= 1e-6
    off_pos = _dev(R.site_layout(case[2].numpy()) == 0)
    assert bool((_bits(d)[off_pos] == 0).all()) and bool((_bits(t)[off_pos] == 0).all())      # exactly +0.0 at every non-positive
    assert bool((d[~off_pos] != 0).all())
    return out, d, t, off_pos


# ------------------------------------------------------------------------------------------------------------ 1. loss
@pytest.mark.parametrize("metric", C.METRICS)
@pytest.mark.parametrize("shape", C.LOSS_SHAPES, ids=_ids3)
def test_loss_against_the_reference(shape, metric):
    from voxelnet_amd import _lib
    case = C.loss_case(shape)
    out, d, t, off_pos = _check_loss(case, shape, metric, 11)
    # two runs are bit-identical; the optional outputs change nothing
    out2, d2, t2 = _raw_loss(case, metric)
    assert torch.equal(_bits(out), _bits(out2)) and torch.equal(_bits(d), _bits(d2)) and torch.equal(_bits(t), _bits(t2))
    fwd, _, _ = _raw_loss(case, metric, with_grad=False, with_target=False)
    assert torch.equal(_bits(out), _bits(fwd))
    only_t, _, t3 = _raw_loss(case, metric, with_grad=False)
    assert torch.equal(_bits(out), _bits(only_t)) and torch.equal(_bits(t), _bits(t3))
    # a NaN in delta and in the logits at a non-positive anchor: nothing changes
    z, delta = case[0].clone(), case[1].clone()
    B, H, W, _ = case[2].shape
    b, a, s = torch.nonzero(torch.from_numpy(R.site_layout(case[2].numpy())) == 0)[3].tolist()
    delta[b, 7 * a + 4, s // W, s % W] = float("nan")
    z[b, a, s] = float("nan")
    out3, d3, t4 = _raw_loss((z, delta) + case[2:], metric)
    assert torch.equal(_bits(out), _bits(out3)) and torch.equal(_bits(d), _bits(d3)) and torch.equal(_bits(t), _bits(t4))
    with pytest.raises(_lib.VoxelnetHipError, match="invalid argument"):
        _raw_loss(case, 2)
    with pytest.raises(_lib.VoxelnetHipError):
        _raw_loss(case, metric, ws_bytes=16)


# ----------------------------------------------------------------------------------------------------------- 2. seams
@pytest.mark.parametrize("metric", C.METRICS)
@pytest.mark.parametrize("shape", list(R.IR.SEAM_CASES), ids=_ids3)
def test_loss_seams_of_the_site_term_scaffold(shape, metric):
    """the two loops of csrc/rpn_common.h's scaffold that no LOSS_SHAPES entry reaches (iou_loss_ref.SEAM_CASES): k_pos_norm's
    second sweep over a sample, and k_site_term_finalize's second slab row per thread with a workgroup that straddles two
    samples.  test_loss_against_the_reference's comparisons and bars."""
    _check_loss(C.seam_case(shape), shape, metric, len(R.IR.SEAM_CASES[shape]))


# ------------------------------------------------------------------------------------------------------ 3. target map
def _decode_np(d, A):
    diag = np.hypot(A[:, 4], A[:, 5])
    return np.stack([d[:, 0] * diag + A[:, 0], d[:, 1] * diag + A[:, 1], d[:, 2] * A[:, 3] + A[:, 2], np.exp(d[:, 3]) * A[:, 3],
                     np.exp(d[:, 4]) * A[:, 4], np.exp(d[:, 5]) * A[:, 5], d[:, 6] + A[:, 6]], axis=1)


@pytest.mark.parametrize("metric", C.METRICS)
@pytest.mark.parametrize("shape", C.LOSS_SHAPES, ids=_ids3)
def test_target_map_against_the_projects_own_iou(shape, metric):
    from voxelnet_amd import _lib
    from voxelnet_amd.iou_loss import METRICS
    z, delta, pos, tgt, anchors = C.loss_case(shape)
    B, H, W = shape[:3]
    idx = torch.nonzero(pos).tolist()
    A = np.stack([anchors.numpy().reshape(H, W, 2, 7)[y, x, a] for _, y, x, a in idx])
    P = _decode_np(np.stack([delta[b, a * 7:a * 7 + 7, y, x].numpy() for b, y, x, a in idx]).astype(np.float64), A)
    G = _decode_np(np.stack([tgt[b, y, x, a * 7:a * 7 + 7].numpy() for b, y, x, a in idx]).astype(np.float64), A)
    n = len(idx)
    pd, gd = torch.from_numpy(P).to(DEV), torch.from_numpy(G).to(DEV)
    table = torch.empty((n, n), dtype=torch.float64, device=DEV)
    _lib.call("vn_box_iou_rotated", pd.data_ptr(), n, gd.data_ptr(), n, METRICS[metric], table.data_ptr(), _lib.raw_stream())
    iou = table.diagonal().cpu().numpy()
    _, _, t = _raw_loss((z, delta, pos, tgt, anchors), metric, with_grad=False)
    t = t.cpu().double().numpy()
    got = np.array([t[b, a, y * W + x] for b, y, x, a in idx])
    e = float((np.abs(got - iou) / iou).max())
    print(f"iou target {shape[:3]} {metric}: max relative error {e:.2e} over {n} positives, IoU in [{iou.min():.3f}, {iou.max():.3f}]")
    assert iou.min() > 0 and iou.max() <= 1 and e <= 1e-6
    assert t.sum() == pytest.approx(got.sum(), rel=1e-12)                                 # nothing anywhere else


@pytest.mark.parametrize("metric", C.METRICS)
def test_an_invalid_pair_scores_zero(metric):
    """a target whose exp overflows: t = 0 there, the loss and the gradient stay finite and match the reference"""
    case, (b, a, s) = C.invalid_case()
    L, mae, grad, t_ref, pairs = R.loss(case[0].numpy(), *case[1:], metric)
    assert t_ref[b, a, s] == 0.0 and pairs[0][1] == 0.0 and math.isfinite(L)
    out, d, t = _raw_loss(case, metric)
    got = out.cpu().double().numpy()
    assert _bits(t)[b, a, s].item() == 0 and bool(torch.isfinite(out).all()) and bool(torch.isfinite(d).all())
    assert abs(got[0] - L) <= 1e-5 * abs(L) and abs(got[1] - mae) <= 1e-5 * abs(mae)
    assert np.abs(d.cpu().double().numpy() - grad).max() <= 1e-5 * np.abs(grad).max()
    q = 1.0 / (1.0 + math.exp(-float(case[0][b, a, s])))
    assert float(d[b, a, s]) == pytest.approx(q / float(case[2][b].sum()), rel=1e-6)      # (q - 0) / P_b


# --------------------------------------------------------------------------------------------------------- 4. autograd
@pytest.mark.parametrize("metric", C.METRICS)
def test_autograd_function_and_no_gradient_into_delta(metric):
    from voxelnet_amd.iou_head import rpn_iou_head_loss
    case = C.loss_case(C.LOSS_SHAPES[1])
    out, d, t = _raw_loss(case, metric)
    off_pos = _dev(R.site_layout(case[2].numpy()) == 0)
    z = _dev(case[0]).requires_grad_(True)
    delta = _dev(case[1]).requires_grad_(True)
    B, H, W, _ = case[2].shape
    loss, mae, t_map = rpn_iou_head_loss(z.view(B, 2, H, W), delta, _dev(case[2]), _dev(case[3]), _dev(case[4]).view(H, W, 2, 7), metric,
                                         return_target=True)
    assert torch.equal(_bits(torch.stack([loss.detach(), mae])), _bits(out)) and not mae.requires_grad and not t_map.requires_grad
    assert torch.equal(_bits(t_map), _bits(t))
    (0.2 * loss + 0.0 * delta.sum()).backward()
    assert torch.allclose(z.grad, 0.2 * d, rtol=1e-6, atol=0) and bool((_bits(z.grad)[off_pos] == 0).all())
    assert not delta.grad.any()                                                           # only the 0 * sum term reached delta
    delta2 = _dev(case[1]).requires_grad_(True)
    l2, _ = rpn_iou_head_loss(z, delta2, _dev(case[2]), _dev(case[3]), _dev(case[4]), metric)
    l2.backward()
    assert delta2.grad is None


# ---------------------------------------------------------------------------------------------------------- 5. rectify
@pytest.mark.parametrize("n", C.RECTIFY_N)
def test_rectify_against_numpy_pow(n):
    from voxelnet_amd import _lib
    from voxelnet_amd.iou_head import rectify_probs
    p, z = C.rectify_case(n)
    pd, zd = _dev(p), _dev(z)
    for alpha in (0.0,) + C.ALPHAS:
        buf, out = _guarded(n)
        _lib.call("vn_iou_rectify_probs", pd.data_ptr(), zd.data_ptr(), n, float(alpha), out.data_ptr(), _lib.raw_stream())
        assert bool((buf[n:] == C.SENTINEL).all()) and torch.equal(_bits(pd), _bits(_dev(p)))
        via = rectify_probs(pd.view(1, 1, n), zd.view(1, 1, n), alpha)
        assert via.shape == (1, 1, n) and torch.equal(_bits(via.view(-1)), _bits(out))
        if alpha == 0.0:
            assert torch.equal(_bits(out), _bits(pd))
            continue
        want = R.rectify(p, z, alpha)
        ulps = np.abs(_ordered(out) - _ordered(torch.from_numpy(want)))
        print(f"rectify n {n} alpha {alpha}: max distance {int(ulps.max())} ulp")
        assert ulps.max() <= 1
    for bad in (-0.1, 1.1, float("nan")):
        with pytest.raises(_lib.VoxelnetHipError, match="invalid argument"):
            _lib.call("vn_iou_rectify_probs", pd.data_ptr(), zd.data_ptr(), n, bad, out.data_ptr(), _lib.raw_stream())
    with pytest.raises(_lib.VoxelnetHipError, match="invalid argument"):
        _lib.call("vn_iou_rectify_probs", pd.data_ptr(), zd.data_ptr(), n, 0.5, pd.data_ptr(), _lib.raw_stream())


# ---------------------------------------------------------------------------------------------------- 6. fused forward
FUSED_SHAPES = tuple(DC.HEAD_SHAPES) + tuple((1, m) for m in C.FUSED_M[:3]) + ((5, 13), (3, 43))          # M = 65, 129: several samples
assert sorted(b * s for b, s in FUSED_SHAPES[3:]) == list(C.FUSED_M)


@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("stride", DC.STRIDES)
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("B,S", FUSED_SHAPES)
def test_fused_forward_equals_two_head_forwards_by_bits(B, S, dtype, stride, with_bias):
    from voxelnet_amd import _lib
    from voxelnet_amd.iou_head import site_heads_forward
    c1, c2 = DC.head_case(B, S), DC.head_case(B, S, seed=12)
    rows = _rows_buffer(c1["x"], dtype, stride, DC.SENTINEL)
    w4 = _dev(np.concatenate([c1["w"], c2["w"]]))
    b4 = _dev(np.concatenate([c1["bias"], c2["bias"]])) if with_bias else None
    singles = []
    for k in range(2):
        o = torch.empty((B, 2, S), dtype=torch.float32, device=DEV)
        _lib.call("vn_dir_head_fwd", rows.data_ptr(), _vn(dtype), stride, w4[2 * k:].data_ptr(), b4[2 * k:].data_ptr() if with_bias else None,
                  B, S, o.data_ptr(), _lib.raw_stream())
        singles.append(o)
    buf, out = _guarded(B * 4 * S)
    _lib.call("vn_site_heads_fwd", rows.data_ptr(), _vn(dtype), stride, w4.data_ptr(), b4.data_ptr() if with_bias else None, 4, B, S,
              out.data_ptr(), _lib.raw_stream())
    out = out.view(B, 4, S)
    assert bool((buf[B * 4 * S:] == DC.SENTINEL).all()) and bool((rows[:, DC.C:] == DC.SENTINEL).all())
    assert torch.equal(_bits(out[:, 0:2]), _bits(singles[0])) and torch.equal(_bits(out[:, 2:4]), _bits(singles[1]))
    buf2, out2 = _guarded(B * 2 * S)
    _lib.call("vn_site_heads_fwd", rows.data_ptr(), _vn(dtype), stride, w4.data_ptr(), b4.data_ptr() if with_bias else None, 2, B, S,
              out2.data_ptr(), _lib.raw_stream())
    assert bool((buf2[B * 2 * S:] == DC.SENTINEL).all()) and torch.equal(_bits(out2.view(B, 2, S)), _bits(singles[0]))
    # the wrapper: two heads, then one
    biases = [b4[:2], b4[2:]] if with_bias else None
    za, zb = site_heads_forward(rows[:, :DC.C], [w4[:2], w4[2:].view(2, DC.C, 1, 1)], biases, B)
    assert torch.equal(_bits(za), _bits(singles[0])) and torch.equal(_bits(zb), _bits(singles[1]))
    (zc,) = site_heads_forward(rows[:, :DC.C], [w4[2:]], [b4[2:]] if with_bias else None, B)
    assert torch.equal(_bits(zc), _bits(singles[1]))


# ------------------------------------------------------------------------------------------------------- 7. round trip
def test_round_trip_a_well_placed_box_wins_the_suppression():
    """The test that fails without the feature.  Anchor A decodes onto the ground truth with p = 0.6; its neighbour B, the
    same box 0.4 m further (rotated IoU with A 0.81 > nms_thres), has p = 0.7; the head says q_A = 0.9, q_B = 0.2.  Ranked by
    p alone the suppression keeps B; ranked by sqrt(p q) it keeps A, scored sqrt(0.54)."""
    from voxelnet_amd.predict import TRAINED_DECODE, BoxDecoder
    anchors = C.round_trip_anchors()
    flat = anchors.reshape(-1, 7)
    dec = BoxDecoder("Car", DEV, anchors=anchors)
    probs, deltas, z = (_dev(a) for a in C.round_trip_maps())
    kw = dict(TRAINED_DECODE, score_thres=C.RT_SCORE_THRES, nms_thres=C.RT_NMS_THRES, top_k=20)
    box_a, box_b = flat[2 * C.RT_SITE_A], flat[2 * C.RT_SITE_B]

    def only(det):
        boxes, scores, counts = det
        assert counts.tolist() == [1]
        return boxes[0, 0].cpu().numpy().astype(np.float64), scores[0, 0]

    without = dec.decode_device(probs, deltas, **kw)
    bx, sc = only(without)
    assert np.abs(bx[[0, 1, 4, 5, 6]] - box_b[[0, 1, 4, 5, 6]]).max() < 1e-5 and float(sc) == float(np.float32(0.7))
    bx, sc = only(dec.decode_device(probs, deltas, **kw, iou_logits=z, iou_rectify=0.5))
    assert np.abs(bx[[0, 1, 4, 5, 6]] - box_a[[0, 1, 4, 5, 6]]).max() < 1e-5
    want = torch.tensor([math.sqrt(0.54)], dtype=torch.float32)
    assert abs(int(_ordered(sc.reshape(1))[0]) - int(_ordered(want)[0])) <= 1, (float(sc), float(want))
    # the default exponent is 0.5; alpha = 0 is the call without the logits, bit for bit
    bx2, sc2 = only(dec.decode_device(probs, deltas, **kw, iou_logits=z))
    assert np.array_equal(bx2, bx) and float(sc2) == float(sc)
    zero = dec.decode_device(probs, deltas, **kw, iou_logits=z, iou_rectify=0.0)
    assert all(torch.equal(_bits(x.float()), _bits(y.float())) for x, y in zip(zero, without))
    # rectify first, then the mask: a masked-out A stays out even at alpha = 1, where p^0 = 1 would bring it back
    mask = torch.ones((1, 4, 4, 2), dtype=torch.uint8, device=DEV)
    mask[0, C.RT_SITE_A // 4, C.RT_SITE_A % 4, 0] = 0
    for alpha in (0.5, 1.0):
        bx, sc = only(dec.decode_device(probs, deltas, **kw, iou_logits=z, iou_rectify=alpha, anchor_mask=mask))
        assert np.abs(bx[[0, 1, 4, 5, 6]] - box_b[[0, 1, 4, 5, 6]]).max() < 1e-5
    assert float(sc) == pytest.approx(0.2, rel=1e-6)                                      # alpha = 1: the score is q_B
    # the first half of the tail on its own: A in front of B, both rectified
    cb, cs, idx, cc = dec.candidates_device(probs, deltas, C.RT_SCORE_THRES, 8, layout="site", iou_logits=z)
    assert cc.tolist() == [2] and idx[0, :2].tolist() == [2 * C.RT_SITE_A, 2 * C.RT_SITE_B]
    boxes_l, scores_l = dec(probs, deltas, **kw, iou_logits=z)
    assert len(boxes_l) == 1 and scores_l[0].tolist() == [float(sc2)]
    with pytest.raises(ValueError, match="site"):
        dec.decode_device(probs, deltas, **dict(kw, layout="flat"), iou_logits=z)
    with pytest.raises(ValueError, match="iou_rectify"):
        dec.decode_device(probs, deltas, **kw, iou_logits=z, iou_rectify=1.5)


# ------------------------------------------------------------------------------------------------------------ 8. model
def _tiny_model(mode, native=True, **kw):
    """test_gpu_dir_head._tiny_model with either head: the golden weights, the 16 x 24 grid, the tiny anchors"""
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
    m.__dict__["_targets"] = TargetGenerator("Car", DEV, anchors=ANCHORS_TINY, keep_heading=bool(kw.get("dir_head")))
    return m


def _same(x, y):
    return torch.equal(_bits(x.detach().float()), _bits(y.detach().float()))


@pytest.mark.parametrize("with_dir", [False, True], ids=["iou", "dir+iou"])
@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_model_zero_weight_head_changes_nothing(golden, mode, with_dir):
    """a head whose loss weight is 0 sends a gradient of zeros, which the backward skips — maps, the five scalars and all
    other gradients are those of the same model without the head, bit for bit (with the direction head on, its logits then
    come from the one-read forward on one side and from vn_dir_head_fwd on the other)"""
    from voxelnet_amd import model as M
    _, _, targets, batch = _tiny(golden)
    try:
        a = _tiny_model(mode, native=False, dir_head=with_dir)
        out_a = a(batch, DEV, targets=targets)
        out_a[2].backward()
        h = _tiny_model(mode, dir_head=with_dir, iou_head=True, iou_head_weight=0.0)
        out_h = h(batch, DEV, targets=targets)
        out_h[2].backward()
        torch.cuda.synchronize()
    finally:
        M.set_precision("bf16")
    assert len(out_a) == len(out_h) == 7
    for i, (x, y) in enumerate(zip(out_a, out_h)):
        assert torch.isfinite(x).all() and _same(x, y), (mode, i)
    ga, gh = dict(a.named_parameters()), dict(h.named_parameters())
    assert len(ga) == 104 + 2 * with_dir and len(gh) == len(ga) + 2
    for k in ga:
        assert ga[k].grad is not None and _same(ga[k].grad, gh[k].grad), (mode, k)
    for k in set(gh) - set(ga):
        assert "iou_conv" in k and gh[k].grad is not None and not gh[k].grad.any(), k
    assert h.last_iou_logits.shape == (2, 2, 8, 12) and h.last_iou_head is not None and a.last_iou_head is None and a.last_iou is None
    if with_dir:
        assert _same(a.last_dir_logits, h.last_dir_logits) and _same(a.last_dir[0], h.last_dir[0])


def test_model_head_against_the_float64_oracle(golden):
    """fp32, iou_head_weight 1.  test_gpu_dir_head.test_model_head_against_the_float64_oracle's reference and bars: the CPU
    oracle's float64 train-mode forward with its taps, a float64 1x1 convolution on cat([deconv3, deconv2, deconv1]) for the
    logits, iou_head_ref's target from the oracle's own regression map (a constant) and its loss joined to the oracle's
    rpn_loss, autograd through the trunk.  Logits 1e-3 relative, scalars 2e-3, head gradients 1e-3 of the maximum, trunk
    gradients 5e-2 relative L2."""
    import torch.nn.functional as F
    from voxelnet_amd import model as M
    feats, coords, targets, batch = _tiny(golden)
    pos_n, neg_n, tgt_n = targets
    try:
        h = _tiny_model("fp32", iou_head=True, iou_head_weight=1.0)
        out = h(batch, DEV, targets=targets)
        out[2].backward()
        torch.cuda.synchronize()
    finally:
        M.set_precision("bf16")
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in tr.make_state_dict("Car").items()}
    dk = ("middle_rpn.iou_conv.conv.weight", "middle_rpn.iou_conv.conv.bias")
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
    t_ref, pairs = R.target_map(reg.detach().numpy(), pos_n, tgt_n, ANCHORS_TINY, "3d")
    l_head, mae = R.loss_torch(logits.reshape(2, 2, -1), t_ref, pos_n)
    ref_out = tr.rpn_loss(prob, reg, pos, neg, tgt)
    (ref_out[0] + 1.0 * l_head).backward()
    l_head, ref_out = l_head.detach(), [o.detach() for o in ref_out]
    ez = float((h.last_iou_logits.detach().cpu().double() - logits.detach()).abs().max() / logits.detach().abs().max())
    print(f"iou logits vs the float64 oracle: {ez:.2e}; L {float(h.last_iou_head[0]):.6f} vs {float(l_head):.6f}, mae "
          f"{float(h.last_iou_head[1]):.4f} vs {float(mae):.4f}; {sum(p[1] > 0 for p in pairs)} of {len(pairs)} targets > 0")
    assert ez < 1e-3 and len(pairs) > 0
    assert abs(float(h.last_iou_head[0]) - float(l_head)) <= 2e-3 * abs(float(l_head))
    np.testing.assert_allclose(float(out[2].detach()), float(ref_out[0] + l_head), rtol=2e-3)
    np.testing.assert_allclose(float(out[3].detach()), float(ref_out[1] + l_head), rtol=2e-3)
    np.testing.assert_allclose(float(out[4].detach()), float(ref_out[2]), rtol=2e-3)       # reg_loss: the head adds nothing to it
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


@pytest.mark.parametrize("with_dir", [False, True], ids=["iou", "dir+iou"])
@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_model_train_step_equals_separate_calls_with_the_head(golden, mode, with_dir):
    """with the head on, train_step takes its separate-calls branch (the head is outside the native executor) and equals
    forward + backward + the optimizer as separate calls bit for bit; the head's loss is part of the result"""
    from voxelnet_amd import model as M
    from voxelnet_amd.optim import ClipSGD
    _, _, targets, batch = _tiny(golden)
    try:
        a = _tiny_model(mode, dir_head=with_dir, iou_head=True)
        assert not a._step_fused_ok(mode, None) and not a._native_ok(mode)
        oa = ClipSGD(a.parameters(), lr=1e-3, max_norm=5.0)
        out_a = a.train_step(batch, DEV, oa, targets=targets)
        b = _tiny_model(mode, dir_head=with_dir, iou_head=True)
        ob = ClipSGD(b.parameters(), lr=1e-3, max_norm=5.0)
        out_b = b(batch, DEV, targets=targets)
        out_b[2].backward()
        ob.step()
        c = _tiny_model(mode, native=False, dir_head=with_dir)
        out_c = c(batch, DEV, targets=targets)
        torch.cuda.synchronize()
    finally:
        M.set_precision("bf16")
    for i, (x, y) in enumerate(zip(out_a, out_b)):
        assert torch.isfinite(x).all() and torch.equal(x, y), (mode, i)
    pa, pb = dict(a.named_parameters()), dict(b.named_parameters())
    assert len(pa) == 106 + 2 * with_dir
    for k in pa:
        assert pa[k].grad is not None and torch.isfinite(pa[k].grad).all() and torch.equal(pa[k].grad, pb[k].grad), (mode, k)
        assert torch.equal(pa[k].detach(), pb[k].detach()), (mode, k)
    assert pa["middle_rpn.iou_conv.conv.weight"].grad.abs().max() > 0
    l_head = float(a.last_iou_head[0])
    va, vc = [float(o.detach()) for o in out_a[2:5]], [float(o.detach()) for o in out_c[2:5]]
    assert l_head > 0 and va[0] == pytest.approx(vc[0] + l_head, rel=1e-5)
    assert va[1] == pytest.approx(vc[1] + l_head, rel=1e-5) and va[2] == vc[2]


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_model_both_heads_share_one_read_of_the_concatenation(golden, mode, monkeypatch):
    """both heads on: ONE vn_site_heads_fwd, no vn_dir_head_fwd, and each head's logits are those of the model that has that
    head alone (vn_dir_head_fwd), bit for bit; the backward is two vn_dir_head_bwd calls"""
    from voxelnet_amd import _lib
    from voxelnet_amd import model as M
    _, _, targets, batch = _tiny(golden)
    names, real = [], _lib.call

    def recording(name, *args):
        names.append(name)
        return real(name, *args)
    try:
        both = _tiny_model(mode, dir_head=True, iou_head=True)
        d, i = _tiny_model(mode, dir_head=True), _tiny_model(mode, iou_head=True)
        assert sorted(d.load_state_dict(both.state_dict(), strict=False).unexpected_keys) == sorted(
            k for k in both.state_dict() if "iou_conv" in k)
        i.load_state_dict(both.state_dict(), strict=False)
        monkeypatch.setattr(_lib, "call", recording)
        out = both(batch, DEV, targets=targets)
        out[2].backward()
        monkeypatch.setattr(_lib, "call", real)
        with torch.no_grad():
            d.detect(batch[2], batch[4])
            i.detect(batch[2], batch[4])
        torch.cuda.synchronize()
    finally:
        M.set_precision("bf16")
    assert names.count("vn_site_heads_fwd") == 1 and "vn_dir_head_fwd" not in names and names.count("vn_dir_head_bwd") == 2
    assert names.index("vn_rpn_dir_loss") < names.index("vn_rpn_iou_head_loss")
    assert _same(both.last_dir_logits, d.last_dir_logits) and _same(both.last_iou_logits, i.last_iou_logits)
    assert both.last_dir_logits.shape == both.last_iou_logits.shape == (2, 2, 8, 12)
    for k in ("middle_rpn.dir_conv.conv.weight", "middle_rpn.iou_conv.conv.weight", "middle_rpn.iou_conv.conv.bias"):
        g = dict(both.named_parameters())[k].grad
        assert g is not None and torch.isfinite(g).all() and g.abs().max() > 0, k


def test_model_evaluate_reaches_rectify_probs(golden, monkeypatch):
    """evaluate(decode=TRAINED_DECODE) and predict(decode=) hand the head's logits to the decoder, which rectifies the scores in
    front of the unchanged tail (and of the anchor mask); a decode that does not read the maps by site is refused; fp32x3 and
    a reducer too"""
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
        h = _tiny_model("bf16", iou_head=True, anchor_area_threshold=0)
        dec = BoxDecoder("Car", DEV, anchors=ANCHORS_TINY)
        ev = DetectionEvaluator("Car", DEV)
        decode = dict(TRAINED_DECODE, score_thres=1e-6)
        monkeypatch.setattr(_lib, "call", recording)
        assert h.evaluate(batches, DEV, evaluator=ev, decoder=dec, decode=decode) is ev
        monkeypatch.setattr(_lib, "call", real)
        for want in ("vn_dir_head_fwd", "vn_iou_rectify_probs", "vn_anchor_mask_probs", "vn_rpn_detect_layout"):
            assert want in names, want
        assert names.index("vn_iou_rectify_probs") < names.index("vn_anchor_mask_probs") < names.index("vn_rpn_detect_layout")
        assert "vn_net_forward" not in names and "vn_site_heads_fwd" not in names and h.training
        with pytest.raises(ValueError, match="site"):
            h.evaluate(batches, DEV, decoder=dec, decode=EVAL_DECODE)
        h.anchor_area_threshold = None
        assert h.evaluate(batches, DEV, decoder=dec, decode=decode).compute()["n_det"] > 0
        h.__dict__["_decoder"] = dec
        with torch.no_grad():
            prob, delta = h.detect(batch[2], batch[4])
        names.clear()
        monkeypatch.setattr(_lib, "call", recording)
        tag, rows = h.predict((batch[0],), prob, delta, decode=dict(decode, top_k=20))
        monkeypatch.setattr(_lib, "call", real)
        assert "vn_iou_rectify_probs" in names and len(rows) == 2 and sum(len(r) for r in rows) > 0
        # the scores are the rectified ones: every one is sqrt(p q) of some anchor
        from voxelnet_amd.iou_head import rectify_probs
        rect = rectify_probs(prob, h.last_iou_logits, 0.5).reshape(2, -1).cpu().numpy()
        for b, r in enumerate(rows):
            assert all(np.float32(float(s)) in rect[b] for s in r[:, 8]), b
        with pytest.raises(ValueError, match="site"):
            h.predict((batch[0],), prob, delta)
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


def test_model_without_the_head_is_untouched_and_checkpoints_round_trip(golden):
    """iou_head=False is the model of before — the same state_dict, the native executor, the one-call step, the same bits —;
    a state_dict with the head round-trips; a head-less checkpoint loads with strict=False, the two new keys missing"""
    from voxelnet_amd import model as M
    _, _, targets, batch = _tiny(golden)
    try:
        a, d = _tiny_model("bf16"), _tiny_model("bf16", iou_head=False)
        assert list(a.state_dict()) == list(d.state_dict()) and not any("iou_conv" in k for k in a.state_dict())
        assert a._native_ok("bf16") and a._step_fused_ok("bf16", None) and d._step_fused_ok("bf16", None)
        out_a, out_d = a.train_step(batch, DEV, None, targets=targets), d.train_step(batch, DEV, None, targets=targets)
        assert all(_same(x, y) for x, y in zip(out_a, out_d))
        assert all(_same(p.grad, q.grad) for p, q in zip(a.parameters(), d.parameters()))
        assert a.last_iou_logits is None and a.last_iou_head is None
        h, h2 = _tiny_model("bf16", iou_head=True), _tiny_model("bf16", iou_head=True)
        with torch.no_grad():
            h2.middle_rpn.iou_conv.conv.weight.add_(1.0)
        assert h2.load_state_dict(h.state_dict()).missing_keys == []
        assert torch.equal(h2.middle_rpn.iou_conv.conv.weight, h.middle_rpn.iou_conv.conv.weight)
        res = h2.load_state_dict(a.state_dict(), strict=False)
        assert sorted(res.missing_keys) == ["middle_rpn.iou_conv.conv.bias", "middle_rpn.iou_conv.conv.weight"]
        res = a.load_state_dict(h.state_dict(), strict=False)
        assert sorted(res.unexpected_keys) == ["middle_rpn.iou_conv.conv.bias", "middle_rpn.iou_conv.conv.weight"]
        with torch.no_grad():
            pa, _ = a.detect(batch[2], batch[4])
            ph, _ = h2.detect(batch[2], batch[4])
        assert a.last_iou_logits is None and h2.last_iou_logits.shape == (2, 2, 8, 12)
        assert torch.isfinite(ph).all() and pa.shape == ph.shape
    finally:
        M.set_precision("bf16")
