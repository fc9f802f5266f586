"""CPU: the direction-classifier head's reference (tests/dir_ref.py) against hand-computed values, the guards of
tests/dir_cases.py asserted on the reference alone (no angle within 1e-6 of a bin edge, no deciding logit within 1e-6 of 0
apart from the one hand-made exact 0), the round trip's frames on the CPU reference tests/kitti_ref.py, and the argument
errors that need no device."""
import ctypes
import math

import numpy as np
import pytest
import torch

import dir_cases as C
import dir_ref as R


def test_reference_against_hand_computed_values():
    pi = math.pi
    assert np.allclose(R.wrap_pi([0.0, -0.1, pi + 0.25, -2 * pi - 0.5, 7.0]), [0.0, pi - 0.1, 0.25, pi - 0.5, 7.0 - 2 * pi])
    # dir_offset pi/4: [pi/4, 5pi/4) is bin 0, [5pi/4, 9pi/4) = [-3pi/4, pi/4) is bin 1
    assert R.dir_bin([0.8, 2.0, 3.9, 4.0, 0.2, 0.0, -1.3, -2.3, -2.4, 0.2 - pi, 0.2 + 2 * pi]).tolist() == [0, 0, 0, 1, 1, 1, 1, 1, 0, 0, 1]
    assert R.dir_bin([0.2, -0.2, 3.0, 3.2, -3.2], 0.0).tolist() == [0, 1, 0, 1, 0]
    for th in (0.2, -1.3, 2.0, 5.5, -7.0):          # a box and its turn by pi always fall into different bins
        assert int(R.dir_bin(th)) != int(R.dir_bin(th + pi)) and int(R.dir_bin(th)) == int(R.dir_bin(th + 2 * pi))
    # decode: the rectified yaw is the heading whenever the logit names the heading's bin, whatever multiple of pi r is off by
    for th in (0.2, -1.3, 2.0, 0.2 - pi, 2.0 - pi):
        for k in (-2, -1, 0, 1, 3):
            z = 4.0 if int(R.dir_bin(th)) else -4.0
            got = float(R.rectify(th + k * pi, z))
            assert math.cos(got - th) > 1 - 1e-12, (th, k, got)
            assert math.cos(float(R.rectify(th + k * pi, -z)) - th) < -1 + 1e-12
    assert float(R.rectify(1.0, 0.0)) == pytest.approx(1.0) and float(R.rectify(1.0, 1e-9)) == pytest.approx(1.0 + pi)
    # the loss on a 1 x 1 map: anchor yaws 0 and pi/2; one positive of bin 1 with logit 0 (log 2), one of bin 0 with logit -30
    anchors = np.zeros((1, 1, 2, 7))
    anchors[0, 0, 1, 6] = pi / 2
    tg = np.zeros((1, 1, 1, 14), dtype=np.float32)
    tg[0, 0, 0, 6], tg[0, 0, 0, 13] = 0.2, 2.0 - pi / 2
    pos = np.ones((1, 1, 1, 2), dtype=np.float32)
    L, acc, g, (hits, n) = R.loss(np.array([[[0.0], [-30.0]]]), pos, tg, anchors)
    assert L == pytest.approx((math.log(2.0) + math.log1p(math.exp(-30.0))) / 2, rel=1e-12)
    assert (hits, n) == (1, 2) and acc == 0.5          # logit 0 means bin 0: wrong for the first, right for the second
    assert g.reshape(-1) == pytest.approx([(0.5 - 1.0) / 2, (1 / (1 + math.exp(30.0))) / 2], rel=1e-9)
    L0, acc0, g0, _ = R.loss(np.array([[[3.0], [3.0]]]), np.zeros_like(pos), tg, anchors)
    assert L0 == 0.0 and acc0 == 0.0 and not g0.any()


@pytest.mark.parametrize("off", C.OFFSETS)
@pytest.mark.parametrize("shape", C.LOSS_SHAPES)
def test_loss_cases_hold_the_guard(shape, off):
    c = C.loss_case(shape)
    gap, z = R.guard(c["logits"], c["pos"], c["targets"], c["anchors"], off, exact_zeros=c["n_exact_zero"])
    print(f"{shape} offset {off:.4f}: smallest edge gap {gap:.3g}, smallest deciding |logit| {z:.3g}")
    pos = R.site_layout(c["pos"])
    if shape == C.LOSS_SHAPES[0]:
        assert pos[-1].sum() == 0 and pos[0].sum() > 0
    assert pos[:, 0].sum() > 0 and pos[:, 1].sum() > 0                       # both rotations
    th = R.site_layout(R.theta_gt(c["targets"], c["anchors"]))[pos != 0]
    quadrants = {int(np.floor(R.wrap_pi(t / 2) * 4 / np.pi)) % 4 for t in th}          # quadrant of theta mod 2 pi
    assert quadrants == {0, 1, 2, 3} and th.max() > 2 * np.pi and th.min() < -2 * np.pi
    bins = R.dir_bin(th, off)
    assert 0 < bins.sum() < bins.size
    z = c["logits"][pos != 0]
    for v in C.HAND_LOGITS:
        assert (z == np.float32(v)).any()


@pytest.mark.parametrize("off", C.OFFSETS)
@pytest.mark.parametrize("shape", list(C.SEAM_CASES))
def test_seam_cases_hold_the_guard(shape, off):
    """the inputs of tests/test_gpu_dir_head.py's seam test, on the reference alone: the positives are exactly where
    dir_cases.SEAM_CASES says and reach the loops they are there for; the angles and logits keep the guard; the loss is
    finite and not 0, with hits and misses"""
    import iou_loss_ref
    assert C.SEAM_CASES == iou_loss_ref.SEAM_CASES          # one set of planted positives for both terms
    B, h, w = shape
    flat = C.SEAM_CASES[shape]
    c = C.seam_case(shape)
    R.guard(c["logits"], c["pos"], c["targets"], c["anchors"], off, exact_zeros=c["n_exact_zero"])
    assert sorted(np.flatnonzero(c["pos"].reshape(-1)).tolist()) == sorted(flat) and c["pos"].sum() == len(flat) <= 12
    sites, per_b, last = B * h * w, h * w * 2, B * h * w * 2 - 1
    assert {0, last} <= set(flat)
    if B == 1:          # the normaliser's second sweep: elements at and beyond 16 x 256, fewer than another full sweep
        assert 16 * 256 < per_b < 2 * 16 * 256 and {16 * 256 - 1, 16 * 256} <= set(flat)
    else:               # a second slab row for finalize thread 0; a workgroup that holds the end of sample 0 and the start of sample 1
        assert (sites + 255) // 256 == 257 and sum(f // 2 >= 256 * 256 for f in flat) >= 2
        assert {2 * (h * w - 1) + 1, 2 * h * w} <= set(flat) and (h * w - 1) // 256 == (h * w) // 256
        p_b = c["pos"].sum(axis=(1, 2, 3)).tolist()
        assert p_b[0] != p_b[1] and min(p_b) >= 1
    L, acc, grad, (hits, n) = R.loss(c["logits"], c["pos"], c["targets"], c["anchors"], off)
    assert math.isfinite(L) and L > 0 and n == len(flat) and 0 < hits < n
    assert np.isfinite(grad).all() and (grad[R.site_layout(c["pos"]) != 0] != 0).all()


def test_rectify_case_holds_the_guard():
    c = C.rectify_case()
    B, K = c["idx"].shape
    assert c["counts"].tolist() == [37, 5, 0, 50] and K == 37
    zeros = 0
    for b in range(B):
        for k in range(min(int(c["counts"][b]), K)):
            n = int(c["idx"][b, k])
            z = float(c["logits"][b, n & 1, n >> 1])
            zeros += z == 0.0
            assert z == 0.0 or abs(z) > R.ZERO
            assert float(R.edge_gap(float(c["boxes"][b, k, 6]))) > R.EDGE
    assert zeros >= 1


def test_head_cases():
    for B, S in C.HEAD_SHAPES:
        for name in C.PATTERNS:
            g, listed = C.grad_pattern(name, B, S)
            M = B * S
            assert listed == sorted(listed) and all(0 <= m < M for m in listed)
            if name == "zero":
                assert listed == [] and not g.any()
            if name == "all":
                assert listed == list(range(M))
            if name == "first_last":
                assert listed == sorted({0, M - 1})
            if name == "g0_zero":
                assert g[M // 2, 0] == 0 and g[M // 2, 1] != 0 and M // 2 in listed
            if name == "spread" and M > 512:
                assert len({m // 256 for m in listed}) >= 3


def test_round_trip_frames_score_bbox_ap_one_on_the_reference():
    """the frames of the round trip (tests/test_gpu_dir_head.py) on tests/kitti_ref.py alone: the exact boxes give `bbox` AP
    1.0 and AOS 1.0 at `all`; the same boxes with every second heading turned by pi keep the AP and lose the AOS"""
    import kitti_ref as K
    frames, boxes = C.round_trip_frames(C.round_trip_anchors())
    assert [len(f) for f in frames] == [4, 2, 0]
    yaws = np.concatenate([b[:, 6] for b in boxes])
    assert np.allclose(np.cos(yaws - np.array(C.ROUND_TRIP_YAWS)), 1.0, atol=1e-9)
    assert float(R.edge_gap(yaws).min()) > 0.1
    assert sorted(R.dir_bin(yaws).tolist()) == [0, 0, 0, 1, 1, 1]
    ref, flipped = K.RefEvaluator("Car"), K.RefEvaluator("Car")
    for lines, bx in zip(frames, boxes):
        det = bx.astype(np.float32)
        scores = [0.99 - 0.01 * i for i in range(len(det))]
        ref.add_frame(det, scores, lines)
        turned = det.copy()
        turned[::2, 6] += np.float32(np.pi)
        flipped.add_frame(turned, scores, lines)
    res, bad = ref.compute(), flipped.compute()
    print("exact boxes:", {k: res[k] for k in ("bbox", "aos", "n_gt")}, "every second heading turned:", bad["aos"])
    assert res["n_gt"]["all"] == 6 and res["bbox"]["all"] == 1.0 and res["aos"]["all"] >= 1.0 - 1e-6
    assert bad["bbox"]["all"] == 1.0 and bad["aos"]["all"] <= 1.0 - 0.2


def test_argument_errors_without_a_device():
    from voxelnet_amd import _lib, dir_head as DH
    from voxelnet_amd import model as M
    lib = _lib.load()
    c_d = ctypes.c_double
    # the library's own checks run before any launch and before any pointer is read
    assert lib.vn_dir_head_fwd(None, _lib.VN_BF16, 768, None, None, 1, 5, None, None) == -1
    assert lib.vn_dir_head_fwd(None, _lib.VN_F32X3S, 1536, None, None, 1, 5, None, None) == -1          # split rows: out of scope
    assert lib.vn_dir_head_bwd_workspace_bytes(2, 70) > 0 and lib.vn_dir_head_bwd_workspace_bytes(0, 70) == 0
    assert lib.vn_dir_head_bwd_workspace_bytes(1 << 20, 1 << 20) == 0
    assert lib.vn_rpn_dir_loss_workspace_bytes(2, 16, 24) > 0 and lib.vn_rpn_dir_loss_workspace_bytes(2, 0, 24) == 0
    assert lib.vn_rpn_dir_loss(None, None, None, None, 2, 16, 24, c_d(math.pi / 4), None, 0, None, None, None) == -1
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.vn_rpn_dir_loss(p, p, p, p, 2, 16, 24, c_d(float("nan")), p, 1 << 20, p, None, None) == -1          # NaN offset
    assert lib.vn_rpn_dir_loss(p, p, p, p, 2, 16, 24, c_d(float("inf")), p, 1 << 20, p, None, None) == -1
    assert lib.vn_rpn_dir_loss(p, p, p, p, 2, 16, 24, c_d(0.0), p, 16, p, None, None) == -3                          # short workspace
    assert lib.vn_boxes_rectify_yaw(p, p, p, p, 2, 37, 129, c_d(0.0), None) == -1                                    # odd n_anchors
    assert lib.vn_boxes_rectify_yaw(p, p, p, p, 2, 37, 128, c_d(float("nan")), None) == -1
    assert lib.vn_boxes_rectify_yaw(None, p, p, p, 2, 37, 128, c_d(0.0), None) == -1
    # the Python layer: CPU tensors raise VoxelnetHipError, bad specs ValueError
    x, w = torch.zeros(5, 768), torch.zeros(2, 768)
    with pytest.raises(_lib.VoxelnetHipError):
        DH.dir_head_forward(x, w, None, 1)
    with pytest.raises(_lib.VoxelnetHipError):
        DH.dir_head_backward(torch.zeros(1, 2, 5), x, w, x.clone())
    with pytest.raises(_lib.VoxelnetHipError):
        DH.rpn_dir_loss(torch.zeros(1, 2, 4), torch.zeros(1, 2, 2, 2), torch.zeros(1, 2, 2, 14), torch.zeros(8, 7, dtype=torch.float64))
    with pytest.raises(_lib.VoxelnetHipError):
        DH.rectify_yaw(torch.zeros(1, 3, 7), torch.zeros(1, 3, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), torch.zeros(1, 2, 4), 8)
    for bad in (float("nan"), float("inf"), "x", None):
        with pytest.raises(ValueError):
            DH.check_spec(0.2, bad)
        with pytest.raises(ValueError):
            DH.check_spec(bad, 0.0)
        with pytest.raises(ValueError):
            M.RPN3D(dir_head=True, dir_offset=bad)
    DH.check_spec(0.0, 0.0)
    with pytest.raises(ValueError):
        DH.rpn_dir_loss(torch.zeros(1, 2, 4), torch.zeros(1, 2, 2, 2), torch.zeros(1, 2, 2, 14), torch.zeros(8, 7), float("nan"))


def test_model_surface_without_a_device():
    """(a) and (g) of the model tests need no device: the default model has no trace of the head, the head adds exactly
    two state_dict keys outside the executor's parameter list, checkpoints travel both ways, and the optimizer's
    no-decay group takes the head's bias."""
    from voxelnet_amd import model as M
    from voxelnet_amd.optim import decay_param_groups
    a, b, h = M.RPN3D(), M.RPN3D(dir_head=False), M.RPN3D(dir_head=True, dir_weight=0.3)
    assert list(a.state_dict()) == list(b.state_dict()) and not any("dir_conv" in k for k in a.state_dict())
    assert not any("dir_conv" in n for n, _ in a.named_modules()) and len(a._flat_params()) == 104
    new = ["middle_rpn.dir_conv.conv.weight", "middle_rpn.dir_conv.conv.bias"]
    assert list(h.state_dict()) == list(a.state_dict()) + new
    assert tuple(h.state_dict()[new[0]].shape) == (2, 768, 1, 1) and tuple(h.state_dict()[new[1]].shape) == (2,)
    assert len(h._flat_params()) == 104 and len(list(h.parameters())) == 106
    assert not any(p is q for p in h._flat_params() for q in h.middle_rpn.dir_conv.parameters())
    assert a._native_ok("bf16") and not h._native_ok("bf16") and not h._native_ok("fp32")
    assert (h.dir_weight, a.dir_head, h.dir_head) == (0.3, False, True) and h.dir_offset == math.pi / 4
    h2 = M.RPN3D(dir_head=True)
    assert h2.load_state_dict(h.state_dict()).missing_keys == []
    assert all(torch.equal(v, h2.state_dict()[k]) for k, v in h.state_dict().items())
    res = h2.load_state_dict(a.state_dict(), strict=False)
    assert sorted(res.missing_keys) == sorted(new) and res.unexpected_keys == []
    with pytest.raises(RuntimeError):
        a.load_state_dict(h.state_dict())
    decay, no_decay = decay_param_groups(h, 0.01)
    bias, weight = h.middle_rpn.dir_conv.conv.bias, h.middle_rpn.dir_conv.conv.weight
    assert any(p is bias for p in no_decay["params"]) and not any(p is bias for p in decay["params"])
    assert any(p is weight for p in decay["params"]) and no_decay["weight_decay"] == 0.0
