"""CPU: the IoU-aware confidence head — tests/iou_head_ref.py against hand values, the guards of
tests/iou_head_cases.py on the reference alone, the library's and the Python layer's argument checks, and the model surface."""
import ctypes
import math

import numpy as np
import pytest
import torch

import iou_head_cases as C
import iou_head_ref as R
import iou_loss_ref as IR


def test_reference_against_hand_computed_values():
    # one site, both rotations positive: rotation 0 predicts its target exactly (IoU 1), rotation 1 is off by half a length
    anchors = IR.small_anchors(1, 1)
    pos = np.ones((1, 1, 1, 2), dtype=np.float32)
    tgt = np.zeros((1, 1, 1, 14), dtype=np.float32)
    delta = np.zeros((1, 14, 1, 1), dtype=np.float32)
    diag = math.hypot(1.6, 3.9)
    delta[0, 7 + 1, 0, 0] = np.float32(1.95 / diag)          # rotation 1 has yaw pi/2: its length lies along y
    d1 = float(delta[0, 8, 0, 0]) * diag
    iou1 = (3.9 - d1) / (3.9 + d1)
    for metric in C.METRICS:
        t, pairs = R.target_map(delta, pos, tgt, anchors, metric)
        assert t.shape == (1, 2, 1) and len(pairs) == 2
        assert t[0, 0, 0] == pytest.approx(1.0, abs=1e-12) and t[0, 1, 0] == pytest.approx(iou1, rel=1e-9)
    z = np.array([[[0.0], [2.0]]], dtype=np.float32)
    L, mae, grad, t, _ = R.loss(z, delta, pos, tgt, anchors, "bev")
    q1 = 1.0 / (1.0 + math.exp(-2.0))
    want = 0.5 * (math.log(2.0) + (2.0 - 2.0 * iou1 + math.log1p(math.exp(-2.0))))
    assert L == pytest.approx(want, rel=1e-12)
    assert mae == pytest.approx(0.5 * (abs(0.5 - t[0, 0, 0]) + abs(q1 - iou1)), rel=1e-12)
    assert grad[0, 0, 0] == pytest.approx(0.5 * (0.5 - t[0, 0, 0]), rel=1e-9) and grad[0, 1, 0] == pytest.approx(0.5 * (q1 - iou1), rel=1e-12)
    # the saturated branches stay finite, and an invalid pair scores 0
    zs = torch.tensor([30.0, -30.0, 800.0, -800.0], dtype=torch.float64)
    b = R.bce(zs, torch.tensor([0.25] * 4, dtype=torch.float64))
    zr = torch.linspace(-40.0, 40.0, 161, dtype=torch.float64)          # (0 among them) the operator is the definition's formula
    assert torch.allclose(R.bce(zr, torch.full_like(zr, 0.3)), R.bce_formula(zr, torch.full_like(zr, 0.3)), rtol=1e-14, atol=1e-300)
    assert torch.isfinite(b).all() and float(b[2]) == pytest.approx(600.0) and float(b[3]) == pytest.approx(200.0)
    tgt2 = tgt.copy()
    tgt2[0, 0, 0, 5] = 800.0
    t2, _ = R.target_map(delta, pos, tgt2, anchors, "3d")
    assert t2[0, 0, 0] == 0.0 and t2[0, 1, 0] > 0
    # the rectified score
    p, zz = np.float32([0.6, 0.7, 0.0, 0.0]), np.float32([math.log(9.0), math.log(0.25), 1.0, 1.0])
    assert np.array_equal(R.rectify(p, zz, 0.0).view(np.uint32), p.view(np.uint32))
    r = R.rectify(p, zz, 0.5)
    assert r[0] == pytest.approx(math.sqrt(0.54), rel=2e-7) and r[1] == pytest.approx(math.sqrt(0.14), rel=2e-7) and r[2] == 0.0
    assert R.rectify(p, zz, 1.0)[3] == pytest.approx(1.0 / (1.0 + math.exp(-1.0)), rel=1e-7)          # 0^0 = 1: why the mask comes last


@pytest.mark.parametrize("metric", C.METRICS)
@pytest.mark.parametrize("shape", C.LOSS_SHAPES, ids=lambda s: "x".join(str(v) for v in s[:3]))
def test_loss_cases_hold_the_guards(shape, metric):
    z, delta, pos, tgt, anchors = C.loss_case(shape)
    L, mae, grad, t, pairs = R.loss(z.numpy(), delta, pos, tgt, anchors, metric)
    assert len(pairs) > 10 and all(0.0 < p[1] <= 1.0 for p in pairs)          # no pair is trivially 0
    m = R.site_layout(pos.numpy()) != 0
    assert math.isfinite(L) and L > 0 and 0 < mae < 1 and (grad[~m] == 0).all() and (grad[m] != 0).all()
    hand = z.numpy()[m][:3]
    assert tuple(hand) == C.HAND_LOGITS
    if shape[3]:
        assert pos[-1].sum() == 0


def test_round_trip_and_rectify_cases_hold_the_guards():
    assert C.round_trip_iou_ab() > 0.5 > C.RT_NMS_THRES
    probs, deltas, z = C.round_trip_maps()
    q = 1.0 / (1.0 + np.exp(-z.astype(np.float64)))
    a, b = (0, 0, C.RT_SITE_A // 4, C.RT_SITE_A % 4), (0, 0, C.RT_SITE_B // 4, C.RT_SITE_B % 4)
    assert q[a] == pytest.approx(0.9, rel=1e-6) and q[b] == pytest.approx(0.2, rel=1e-6)
    assert probs[b] > probs[a] > C.RT_SCORE_THRES                                # without the head B wins
    r = R.rectify(probs, z, 0.5)
    assert r[a] > r[b] > C.RT_SCORE_THRES and np.sort(r.reshape(-1))[-3] < C.RT_SCORE_THRES      # with it A wins; nobody else enters
    assert R.rectify(probs, z, 1.0)[b] > C.RT_SCORE_THRES and np.sort(R.rectify(probs, z, 1.0).reshape(-1))[-3] < C.RT_SCORE_THRES
    for n in C.RECTIFY_N:
        p, zz = C.rectify_case(n)
        assert p.shape == zz.shape == (n,) and (p >= 0).all() and (p <= 1).all() and np.abs(zz).max() == 30.0
        if n > 8:
            assert {0.0, 1.0, float(np.float32(1.4e-45))} <= set(float(v) for v in p)


def test_argument_errors_without_a_device():
    from voxelnet_amd import _lib, iou_head as IH
    from voxelnet_amd import model as M
    from voxelnet_amd.predict import LAYOUTS
    lib = _lib.load()
    c_d = ctypes.c_double
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    q = ctypes.cast(ctypes.addressof(buf) + 16, ctypes.c_void_p)
    assert lib.vn_rpn_iou_head_loss_workspace_bytes(2, 16, 24) > 0 and lib.vn_rpn_iou_head_loss_workspace_bytes(2, 0, 24) == 0
    assert lib.vn_rpn_iou_head_loss_workspace_bytes(2, 16, 24) == lib.vn_rpn_dir_loss_workspace_bytes(2, 16, 24)
    assert lib.vn_rpn_iou_head_loss(None, None, None, None, None, 2, 16, 24, 1, None, 0, None, None, None, None) == -1
    assert lib.vn_rpn_iou_head_loss(p, p, p, p, p, 2, 16, 24, 2, p, 1 << 20, p, None, None, None) == -1          # unknown metric
    assert lib.vn_rpn_iou_head_loss(p, p, p, p, p, 2, 16, 24, 1, p, 16, p, None, None, None) == -3                # short workspace
    for bad in (-0.1, 1.1, float("nan"), float("inf")):
        assert lib.vn_iou_rectify_probs(p, p, 4, c_d(bad), q, None) == -1
    assert lib.vn_iou_rectify_probs(p, p, 4, c_d(0.5), p, None) == -1                                             # out aliases probs
    assert lib.vn_iou_rectify_probs(None, p, 4, c_d(0.5), q, None) == -1 and lib.vn_iou_rectify_probs(p, p, 0, c_d(0.5), q, None) == -1
    assert lib.vn_site_heads_fwd(None, _lib.VN_BF16, 768, None, None, 4, 1, 5, None, None) == -1
    assert lib.vn_site_heads_fwd(p, _lib.VN_BF16, 768, p, None, 3, 1, 5, p, None) == -1                           # n_out not 2 / 4
    assert lib.vn_site_heads_fwd(p, _lib.VN_F32X3S, 1536, p, None, 4, 1, 5, p, None) == -1                        # split rows
    # the Python layer: CPU tensors raise VoxelnetHipError, bad specs ValueError
    x, w = torch.zeros(5, 768), torch.zeros(2, 768)
    with pytest.raises(_lib.VoxelnetHipError):
        IH.site_heads_forward(x, [w, w], None, 1)
    with pytest.raises(ValueError):
        IH.site_heads_forward(x, [w, w, w], None, 1)
    with pytest.raises(_lib.VoxelnetHipError):
        IH.rpn_iou_head_loss(torch.zeros(1, 2, 4), torch.zeros(1, 14, 2, 2), torch.zeros(1, 2, 2, 2), torch.zeros(1, 2, 2, 14),
                             torch.zeros(8, 7, dtype=torch.float64))
    with pytest.raises(_lib.VoxelnetHipError):
        IH.rectify_probs(torch.zeros(1, 2, 4), torch.zeros(1, 2, 4), 0.5)
    for bad in (-0.1, 1.1, float("nan"), "x", None):
        with pytest.raises(ValueError):
            IH.check_spec(1.0, bad, "3d")
        with pytest.raises(ValueError):
            IH.rectify_probs(torch.zeros(1, 2, 4), torch.zeros(1, 2, 4), bad)
        with pytest.raises(ValueError):
            M.RPN3D(iou_head=True, iou_rectify=bad)
    for bad in (float("nan"), float("inf"), "x", None):
        with pytest.raises(ValueError):
            IH.check_spec(bad, 0.5, "3d")
    with pytest.raises(ValueError):
        IH.check_spec(1.0, 0.5, "giou")
    with pytest.raises(ValueError):
        M.RPN3D(iou_head=True, iou_head_metric="x")
    IH.check_spec(0.0, 0.0, "bev")
    IH.check_spec(2.0, 1.0, "3d")
    assert M.RPN3D.__init__.__kwdefaults__["iou_head"] is False
    assert set(LAYOUTS) == {"flat", "site"}


def test_decoder_refuses_iou_logits_outside_the_site_layout():
    """the decoder's argument errors come before anything touches a device: a decoder object without one"""
    from voxelnet_amd import _lib
    from voxelnet_amd.predict import BoxDecoder
    dec = BoxDecoder.__new__(BoxDecoder)
    dec.layout, dec.n_anchors = "flat", 32
    probs, deltas, z = (torch.from_numpy(a) for a in C.round_trip_maps())
    for call in (lambda **kw: dec.decode_device(probs, deltas, 0.1, **kw), lambda **kw: dec.candidates_device(probs, deltas, 0.1, 8, **kw),
                 lambda **kw: dec(probs, deltas, 0.1, **kw)):
        with pytest.raises(ValueError, match="site"):
            call(iou_logits=z)                                     # the decoder's own layout is "flat"
        with pytest.raises(ValueError, match="site"):
            call(iou_logits=z, layout="flat")
        with pytest.raises(_lib.VoxelnetHipError):
            call(iou_logits=z, layout="site")                      # CPU tensors: no CPU path


def test_model_surface_without_a_device():
    """the default model has no trace of the head; the head adds exactly two state_dict keys outside the executor's parameter
    list, behind the direction head's; checkpoints travel both ways; old pickles read the class-level defaults"""
    from voxelnet_amd import model as M
    a, b, h = M.RPN3D(), M.RPN3D(iou_head=False), M.RPN3D(iou_head=True, iou_head_weight=0.7, iou_rectify=0.25, iou_head_metric="bev")
    assert list(a.state_dict()) == list(b.state_dict()) and not any("iou_conv" in k for k in a.state_dict())
    assert not any("iou_conv" in n for n, _ in a.named_modules()) and len(a._flat_params()) == 104
    new = ["middle_rpn.iou_conv.conv.weight", "middle_rpn.iou_conv.conv.bias"]
    assert list(h.state_dict()) == list(a.state_dict()) + new
    assert tuple(h.state_dict()[new[0]].shape) == (2, 768, 1, 1) and not h.state_dict()[new[1]].any()          # the bias starts at 0
    assert len(h._flat_params()) == 104 and len(list(h.parameters())) == 106
    assert a._native_ok("bf16") and not h._native_ok("bf16") and not h._native_ok("fp32") and not h._step_fused_ok("bf16", None)
    assert (h.iou_head_weight, h.iou_rectify, h.iou_head_metric, a.iou_head, h.iou_head) == (0.7, 0.25, "bev", False, True)
    assert (a.iou_head_weight, a.iou_rectify, a.iou_head_metric) == (1.0, 0.5, "3d") and "iou_head_weight" not in a.__dict__
    both = M.RPN3D(dir_head=True, iou_head=True)
    assert list(both.state_dict())[-4:] == ["middle_rpn.dir_conv.conv.weight", "middle_rpn.dir_conv.conv.bias"] + new
    h2 = M.RPN3D(iou_head=True)
    assert h2.load_state_dict(h.state_dict()).missing_keys == []
    assert all(torch.equal(v, h2.state_dict()[k]) for k, v in h.state_dict().items())
    res = h2.load_state_dict(a.state_dict(), strict=False)
    assert sorted(res.missing_keys) == sorted(new) and res.unexpected_keys == []
    res = a.load_state_dict(h.state_dict(), strict=False)
    assert res.missing_keys == [] and sorted(res.unexpected_keys) == sorted(new)
    with pytest.raises(RuntimeError):
        a.load_state_dict(h.state_dict())
    for k in ("last_iou_head", "last_iou_logits"):
        assert k in M.RPN3D._RUNTIME_KEYS and getattr(a, k) is None
    h.last_iou_logits = torch.zeros(1)
    assert "last_iou_logits" not in h.__getstate__() and "last_iou" in M.RPN3D._RUNTIME_KEYS
    old = M.RPN3D.__new__(M.RPN3D)          # a pickle from before the head: nothing of it in __dict__
    assert old.iou_head is False and old.iou_rectify == 0.5
