"""CPU: Soft-NMS without a GPU — the reference tests/soft_nms_ref.py on hand cases and against
tests/detect_ref.nms, the host-side argument checks of vn_box_soft_nms (status codes, before any launch), and the Python layer's
argument checks."""
import ctypes
import dataclasses
import inspect
import math

import numpy as np
import pytest
import torch

import detect_ref as D
import soft_nms_ref as S
import tta_ref as T

EINVAL, EWORKSPACE = -1, -3
BOX = [20.0, 3.0, -1.0, 1.5, 1.6, 3.9, 0.3]


@pytest.fixture(autouse=True)
def _the_reference_numbers_its_modes_as_the_abi_does():
    from voxelnet_amd import _lib
    assert (S.HARD, S.LINEAR, S.GAUSSIAN, S.BEV, S.D3) == (_lib.VN_SOFT_HARD, _lib.VN_SOFT_LINEAR, _lib.VN_SOFT_GAUSSIAN, _lib.VN_SOFT_BEV,
                                                          _lib.VN_SOFT_3D)


def _rows(*offsets):
    return np.array([[BOX[0] + dx, BOX[1] + dy] + BOX[2:] for dx, dy in offsets], dtype=np.float32)


# ------------------------------------------------------------------------------------------- the reference itself
def test_reference_two_identical_boxes():
    boxes, scores = _rows((0, 0), (0, 0)), np.array([0.75, 0.5], dtype=np.float32)
    u = S.R.iou_pair(boxes[0].astype(np.float64), boxes[1].astype(np.float64))
    assert abs(u[0] - 1.0) < 1e-12 and abs(u[1] - 1.0) < 1e-12
    for metric, uu in ((S.BEV, u[0]), (S.D3, u[1])):
        g = S.soft_nms(boxes, scores, 2, S.GAUSSIAN, metric, 0.3, 0.5, 0.0, 20)
        assert g["keep"] == [0, 1] and g["w"][0] == 0.75 and g["decays"] == [0, 1]
        assert g["w"][1] == 0.5 * math.exp(-(uu * uu) / 0.5) and abs(g["w"][1] - 0.5 * math.exp(-2.0)) < 1e-12
        assert g["bound"][0] == 0.0 and abs(g["bound"][1] - 4.0 * S.IOU_BAR) < 1e-18
        lin = S.soft_nms(boxes, scores, 2, S.LINEAR, metric, 0.3, 0.5, 0.0, 20)
        assert lin["keep"] == [0, 1] and lin["w"][1] == 0.5 * (1.0 - uu) and abs(lin["w"][1]) < 1e-12          # s * 0
        h = S.soft_nms(boxes, scores, 2, S.HARD, metric, 0.3, 0.5, 0.0, 20)
        assert h["keep"] == [0] and h["w"] == [0.75]
    # the larger score is picked first wherever it stands; equal scores: the smaller row
    assert S.soft_nms(boxes, scores[::-1].copy(), 2, S.GAUSSIAN, S.BEV, 0.3, 0.5, 0.0, 20)["keep"] == [1, 0]
    assert S.soft_nms(boxes, np.float32([0.5, 0.5]), 2, S.GAUSSIAN, S.BEV, 0.3, 0.5, 0.0, 20)["keep"] == [0, 1]
    # the walk stops at post_top_k BEFORE the decay
    assert S.soft_nms(boxes, scores, 2, S.GAUSSIAN, S.BEV, 0.3, 0.5, 0.0, 1)["keep"] == [0]


def test_reference_disjoint_boxes_keep_their_scores():
    boxes = _rows((0, 0), (10, 0), (0, 10), (30, 30))
    scores = np.array([0.5, 0.875, -0.0, 0.25], dtype=np.float32)
    for method in (S.HARD, S.LINEAR, S.GAUSSIAN):
        for metric in (S.BEV, S.D3):
            out = S.soft_nms(boxes, scores, 4, method, metric, 0.3, 0.5, -1.0, 20)
            assert out["keep"] == [1, 0, 3, 2] and out["decays"] == [0, 0, 0, 0]
            assert np.array_equal(np.float32(out["w"]).view(np.uint32), scores[[1, 0, 3, 2]].view(np.uint32))
            assert out["gap2"] == math.inf
    # n cuts the pool; an invalid row and a non-finite score are never picked
    assert S.soft_nms(boxes, scores, 2, S.GAUSSIAN, S.BEV, 0.3, 0.5, -1.0, 20)["keep"] == [1, 0]
    assert S.soft_nms(boxes, scores, 9, S.GAUSSIAN, S.BEV, 0.3, 0.5, -1.0, 20)["keep"] == [1, 0, 3, 2]
    assert S.soft_nms(boxes, scores, -1, S.GAUSSIAN, S.BEV, 0.3, 0.5, -1.0, 20)["keep"] == []
    bad = boxes.copy()
    bad[1, 5] = 0.0
    assert S.soft_nms(bad, np.float32([0.5, 0.875, np.nan, np.inf]), 4, S.GAUSSIAN, S.BEV, 0.3, 0.5, -1.0, 20)["keep"] == [0]


def test_reference_min_score_stops_the_walk():
    boxes, scores = _rows((0, 0), (0.25, 0), (10, 0)), np.array([0.75, 0.625, 0.25], dtype=np.float32)
    u = S.R.iou_pair(boxes[0].astype(np.float64), boxes[1].astype(np.float64))[0]
    decayed = 0.625 * math.exp(-(u * u) / 0.5)
    assert 0.5 < u < 1 and decayed < 0.25
    out = S.soft_nms(boxes, scores, 3, S.GAUSSIAN, S.BEV, 0.3, 0.5, 0.2, 20)
    assert out["keep"] == [0, 2] and out["w"] == [0.75, 0.25]          # row 1 fell to `decayed`, below the floor, behind row 2
    assert abs(out["floor_gap"] - abs(decayed - 0.2) / 0.2) < 1e-12
    assert S.soft_nms(boxes, scores, 3, S.GAUSSIAN, S.BEV, 0.3, 0.5, 0.0, 20)["keep"] == [0, 2, 1]
    assert S.soft_nms(boxes, scores, 3, S.GAUSSIAN, S.BEV, 0.3, 0.5, 0.75, 20)["keep"] == [0]          # w >= min_score keeps
    assert S.soft_nms(boxes, scores, 3, S.GAUSSIAN, S.BEV, 0.3, 0.5, 0.76, 20)["keep"] == []
    # linear leaves an overlap at or below iou_thres alone
    assert S.soft_nms(boxes, scores, 3, S.LINEAR, S.BEV, 0.99, 0.5, 0.0, 20)["w"] == [0.75, 0.625, 0.25]


@pytest.mark.parametrize("K, P, seed", [(64, 20, 2), (257, 64, 3)])
def test_reference_hard_mode_is_the_greedy_nms(K, P, seed):
    boxes, scores, counts = T.clustered_pools(seed, 1, 1, K, [(1.0, 0.0, 1.0)])
    assert (np.diff(scores[0, 0, :counts[0, 0]]) <= 0).all()
    n = int(counts[0, 0])
    keep, _ = D.nms(boxes[0, 0, :n], D.ROTATED, 0.1, P)
    out = S.soft_nms(boxes[0, 0], scores[0, 0], n, S.HARD, S.BEV, 0.1, 0.5, 0.05, P)
    assert out["keep"] == [int(k) for k in keep] and len(keep) >= 2
    assert np.array_equal(np.float32(out["w"]), scores[0, 0][keep]) and not any(out["decays"])


# ------------------------------------------------------------------------------------------- the C ABI's checks
def _buf(n=64):
    return ctypes.cast(ctypes.create_string_buffer(n), ctypes.c_void_p)


def test_soft_nms_refuses_every_limit_before_any_launch():
    from voxelnet_amd import _lib
    lib = _lib.load()
    q = lib.vn_box_soft_nms_workspace_bytes
    assert q(1, 1) > 0 and q(3, 4096) > 0
    for B, K in [(0, 1), (-1, 1), (1, 0), (1, -1), (1, 4097)]:
        assert q(B, K) == 0, (B, K)
    p = _buf()          # host memory: every call below must return before it would touch it on the device

    def call(B=1, K=8, method=2, metric=0, thres=0.3, sigma=0.5, floor=0.05, P=4, ws=1 << 12, null=None):
        a = [p, p, p, B, K, method, metric, thres, sigma, floor, P, p, p, p, p, ws, None]
        if null is not None:
            a[null] = None
        return lib.vn_box_soft_nms(*a)
    for kw in [dict(B=0), dict(B=-2), dict(K=0), dict(K=4097), dict(P=0), dict(P=65), dict(method=3), dict(method=-1), dict(metric=2),
               dict(metric=-1), dict(thres=-0.01), dict(thres=1.01), dict(thres=math.nan), dict(thres=math.inf), dict(sigma=0.0),
               dict(sigma=-1.0), dict(sigma=math.inf), dict(sigma=math.nan), dict(floor=math.nan), dict(floor=math.inf),
               dict(floor=-math.inf), dict(method=0, sigma=0.0)]:
        assert call(**kw) == EINVAL, kw
    for null in (0, 1, 2, 11, 12, 13, 14):
        assert call(null=null) == EINVAL, null
    assert call(ws=q(1, 8) - 1) == EWORKSPACE
    assert lib.vn_box_soft_nms(None, None, None, 1, 1, 0, 0, 0.3, 0.5, 0.0, 1, None, None, None, None, 0, None) == EINVAL
    assert (_lib.VN_SOFT_HARD, _lib.VN_SOFT_LINEAR, _lib.VN_SOFT_GAUSSIAN, _lib.VN_SOFT_BEV, _lib.VN_SOFT_3D) == (0, 1, 2, 0, 1)
    assert lib.vn_abi_version() == 4


# ------------------------------------------------------------------------------------------- the Python layer
def test_soft_nms_object_checks_its_arguments():
    from voxelnet_amd import predict as PR
    s = PR.SoftNMS()
    assert s == PR.SoftNMS("gaussian", 0.5, 0.3, "bev", None)
    assert (PR.SOFT_METHODS, PR.SOFT_METRICS) == (dict(hard=S.HARD, linear=S.LINEAR, gaussian=S.GAUSSIAN), {"bev": S.BEV, "3d": S.D3})
    with pytest.raises(dataclasses.FrozenInstanceError):
        s.sigma = 1.0
    PR.SoftNMS(method="linear", iou_thres=0, metric="3d", min_score=-1.0)
    PR.SoftNMS(method="hard", iou_thres=1)
    for kw in [dict(method="soft"), dict(method=2), dict(metric="standup"), dict(sigma=0.0), dict(sigma=-0.5), dict(sigma=math.inf),
               dict(sigma=math.nan), dict(sigma="0.5"), dict(iou_thres=-0.1), dict(iou_thres=1.5), dict(iou_thres=math.nan),
               dict(min_score=math.nan), dict(min_score=math.inf), dict(min_score="0.1")]:
        with pytest.raises(ValueError):
            PR.SoftNMS(**kw)


def test_cpu_tensors_raise_and_arguments_are_checked():
    from voxelnet_amd import _lib
    from voxelnet_amd import predict as PR
    b, s, c = torch.zeros((1, 4, 7)), torch.zeros((1, 4)), torch.zeros(1, dtype=torch.int32)
    with pytest.raises(_lib.VoxelnetHipError):
        PR.soft_nms_device(b, s, c, PR.SoftNMS(), 4, min_score=0.1)
    with pytest.raises(ValueError):
        PR.soft_nms_device(b, s, c, "gaussian", 4, min_score=0.1)
    for kw in [dict(), dict(min_score=math.nan), dict(min_score="0.1")]:          # neither says where the walk stops; not a number
        with pytest.raises(ValueError):
            PR.soft_nms_device(b, s, c, PR.SoftNMS(), 4, **kw)
    with pytest.raises(_lib.VoxelnetHipError):
        PR.soft_nms_device(b, s, c, PR.SoftNMS(min_score=0.1), 4)
    # gather_kept with the kept scores: they come back in place of the pool's, zero past the count
    boxes = torch.arange(2 * 5 * 7, dtype=torch.float32).view(2, 5, 7)
    scores = torch.arange(10, dtype=torch.float32).view(2, 5)
    keep = torch.tensor([[3, 1, -1], [4, -1, -1]], dtype=torch.int32)
    kc = torch.tensor([2, 0], dtype=torch.int32)
    ks = torch.tensor([[0.75, 0.5, 0.0], [0.25, 0.0, 0.0]])
    gb, gs, gc = PR.gather_kept(boxes, scores, keep, kc, keep_scores=ks)
    assert gs.tolist() == [[0.75, 0.5, 0.0], [0.0, 0.0, 0.0]] and gc is kc
    pb, ps, _ = PR.gather_kept(boxes, scores, keep, kc)
    assert torch.equal(gb, pb) and ps.tolist() == [[3.0, 1.0, 0.0], [0.0, 0.0, 0.0]] and torch.equal(gb[0, 0], boxes[0, 3])


def test_decode_signatures_take_soft_nms():
    from voxelnet_amd import model as M
    from voxelnet_amd.predict import BoxDecoder, gather_kept, soft_nms_device
    for fn in (BoxDecoder.decode_device, BoxDecoder.__call__):
        assert inspect.signature(fn).parameters["soft_nms"].default is None
        assert list(inspect.signature(fn).parameters)[-2:] == ["vote", "soft_nms"]          # the calls of before still bind
    assert inspect.signature(gather_kept).parameters["keep_scores"].default is None
    assert list(inspect.signature(soft_nms_device).parameters) == ["boxes", "scores", "counts", "soft", "top_k", "min_score"]
    assert "soft_nms" in inspect.getsource(M.RPN3D._tta_decode)
