"""CPU: the evaluation tail's host side — the reference tests/detect_ref.py on hand-made cases, and
the argument checks and workspace queries of vn_rpn_select_decode, vn_box_nms and vn_rpn_detect through ctypes (status
codes, no GPU)."""
import ctypes
import math

import numpy as np
import pytest

import detect_ref as D

CAR = [20.0, 3.0, -1.6, 1.5, 1.6, 3.9, 0.0]          # x y z h w l r


def _boxes(rows):
    return np.array(rows, dtype=np.float32).reshape(-1, 7)


def _moved(dx=0.0, dy=0.0, r=None, base=CAR):
    q = list(base)
    q[0] += dx
    q[1] += dy
    if r is not None:
        q[6] = r
    return q


@pytest.mark.parametrize("mode", [D.STANDUP, D.ROTATED])
def test_identical_boxes_keep_one(mode):
    keep, gap = D.nms(_boxes([CAR] * 7), mode, 0.1, 20)
    assert keep == [0] and abs(gap - 0.9) < 1e-12


@pytest.mark.parametrize("mode", [D.STANDUP, D.ROTATED])
def test_chain_is_greedy_not_suppressed_by_anyone(mode):
    """A kills B (IoU 1/3); B would kill C (IoU 0.23) but is dead; A and C do not touch: A and C are kept"""
    a, b, c = CAR, _moved(dx=1.95), _moved(dx=4.4)
    assert D.nms(_boxes([a, b, c]), mode, 0.1, 20)[0] == [0, 2]
    assert D.nms(_boxes([b, a, c]), mode, 0.1, 20)[0] == [0]          # walked from B, both go


def test_side_by_side_at_45_degrees():
    """two cars at yaw pi/4, 2.4 m apart across their heading: the footprints do not touch, the stand-up squares overlap
    at IoU ~0.19 > 0.1"""
    r = math.pi / 4
    a = _moved(r=r)
    b = _moved(dx=-2.4 * math.sin(r), dy=2.4 * math.cos(r), r=r)
    keep, gap = D.nms(_boxes([a, b]), D.ROTATED, 0.1, 20)
    assert keep == [0, 1] and abs(gap - 0.1) < 1e-12          # IoU exactly 0
    keep, gap = D.nms(_boxes([a, b]), D.STANDUP, 0.1, 20)
    assert keep == [0] and 0.08 < gap < 0.10                  # IoU 0.19


def test_invalid_boxes():
    nan = _moved()
    nan[0] = float("nan")
    flat = _moved()
    flat[4] = 0.0
    rows = _boxes([flat, nan, CAR, _moved(dx=0.1)])
    # rotated: never kept, suppress nothing
    assert D.nms(rows, D.ROTATED, 0.1, 20)[0] == [2]
    assert D.nms(_boxes([CAR, nan, flat]), D.ROTATED, 0.1, 20)[0] == [0]
    # stand-up (the reference's rule, utils.py:519-551): a zero-width rectangle has IoU 0 with everything, is kept and
    # suppresses nothing; a NaN IoU suppresses, so a NaN row goes with the first kept row before it, and a leading NaN row
    # is kept and takes every later row with it
    assert D.nms(rows, D.STANDUP, 0.1, 20)[0] == [0, 2]
    assert D.nms(_boxes([CAR, nan, _moved(dx=30.0)]), D.STANDUP, 0.1, 20)[0] == [0, 2]
    assert D.nms(_boxes([nan, CAR, _moved(dx=30.0)]), D.STANDUP, 0.1, 20)[0] == [0]


@pytest.mark.parametrize("mode", [D.STANDUP, D.ROTATED])
def test_walk_stops_at_the_cap(mode):
    rows = _boxes([_moved(dx=6.0 * k) for k in range(10)])
    assert D.nms(rows, mode, 0.1, 20)[0] == list(range(10))
    assert D.nms(rows, mode, 0.1, 4)[0] == [0, 1, 2, 3]
    assert D.nms(rows, mode, 0.1, 1)[0] == [0]
    assert D.nms(_boxes([]), mode, 0.1, 4) == ([], float("inf"))


def test_negative_threshold_suppresses_disjoint_boxes_too():
    """IoU 0 <= -0.5 is false: with a negative threshold every later row goes, touching or not"""
    rows = _boxes([_moved(dx=50.0 * k) for k in range(4)])
    for mode in (D.STANDUP, D.ROTATED):
        assert D.nms(rows, mode, -0.5, 20)[0] == [0]


def test_select_order_ties_and_nan():
    p = np.array([0.5, 0.9, 0.9, np.nan, 0.2, 0.9, -0.0, 0.0, 1.0], dtype=np.float32)
    assert D.select(p, 0.5, 10).tolist() == [8, 5, 2, 1, 0]          # equal scores: the larger index first
    assert D.select(p, 0.5, 3).tolist() == [8, 5, 2]
    assert D.select(p, 0.0, 10).tolist() == [8, 5, 2, 1, 0, 4, 7, 6]  # -0.0 >= 0.0, and ties with +0.0 by index
    assert D.select(p, 2.0, 10).tolist() == []
    assert D.select(p, -np.inf, 20).tolist() == [8, 5, 2, 1, 0, 4, 7, 6]          # the NaN never


def test_decode_restates_the_oracle():
    from oracle import predict as op
    from oracle import targets as ot
    rng = np.random.default_rng(3)
    anchors = ot.generate_anchors("Car")[:6, :5]
    deltas = (rng.standard_normal((1, 14, 6, 5)) * 0.3).astype(np.float32)
    idx = np.array([59, 0, 17, 17, 33])
    assert np.array_equal(D.decode(deltas[0], anchors, idx), op.deltas_to_boxes_3d(deltas, anchors)[0][idx])


def test_detect_with_the_reference_settings_is_the_oracle():
    """stand-up, pre = post = 20, 0.96 / 0.1: detect_ref.detect is oracle/predict.py's predict_boxes"""
    from oracle import predict as op
    from oracle import targets as ot
    from test_oracle_predict import maps
    probs, deltas = maps()
    anchors = ot.generate_anchors("Car")
    rb, rs = op.predict_boxes(probs, deltas, anchors)
    for b in range(probs.shape[0]):
        boxes, scores = D.detect(probs[b], deltas[b], anchors, op.SCORE_THRES, 20, D.STANDUP, op.NMS_THRES, 20)
        assert np.array_equal(scores, rs[b]) and np.array_equal(boxes, rb[b].reshape(-1, 7)), b


def test_three_clustered_cars_need_a_wider_pool():
    """the first table of the issue: three well-separated cars, 30 near-duplicates each at 0.99.., 0.98.., 0.97.."""
    rng = np.random.default_rng(0)
    rows, scores = [], []
    for c, (x, y) in enumerate([(15.0, -10.0), (35.0, 4.0), (55.0, 20.0)]):
        for k in range(30):
            rows.append(_moved(dx=x - CAR[0] + rng.uniform(-0.1, 0.1), dy=y - CAR[1] + rng.uniform(-0.1, 0.1), r=0.3))
            scores.append(0.99 - 0.01 * c + 1e-4 * k)
    order = np.argsort(-np.array(scores), kind="stable")
    rows = _boxes(rows)[order]
    assert len(D.nms(rows[:20], D.STANDUP, 0.1, 20)[0]) == 1
    assert len(D.nms(rows[:90], D.STANDUP, 0.1, 20)[0]) == 3
    assert len(D.nms(rows[:90], D.ROTATED, 0.1, 20)[0]) == 3


# ------------------------------------------------------------------------------------------ C ABI, no GPU
EINVAL, EWORKSPACE = -1, -3


def _buf():
    buf = (ctypes.c_double * 64)()
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def test_workspace_queries():
    from voxelnet_amd import _lib
    lib = _lib.load()
    assert _lib.VN_NMS_STANDUP == 0 and _lib.VN_NMS_ROTATED == 1 and _lib.VN_DETECT_MAX_PRE == 4096
    sel = lib.vn_rpn_select_decode_workspace_bytes(2, 70400, 1024)
    assert sel >= 2 * 4 + 2 * 70400 * 8
    assert lib.vn_rpn_select_decode_workspace_bytes(2, 70400, 0) == 0
    assert lib.vn_rpn_select_decode_workspace_bytes(2, 70400, 4097) == 0
    assert lib.vn_rpn_select_decode_workspace_bytes(0, 70400, 20) == 0
    assert lib.vn_rpn_select_decode_workspace_bytes(2, 0, 20) == 0
    assert lib.vn_rpn_select_decode_workspace_bytes(2, 1 << 30, 20) == 0
    nms = lib.vn_box_nms_workspace_bytes(2, 4096)
    assert nms > 0 and lib.vn_box_nms_workspace_bytes(2, 1) > 0
    assert lib.vn_box_nms_workspace_bytes(2, 0) == 0 and lib.vn_box_nms_workspace_bytes(2, 4097) == 0
    assert lib.vn_box_nms_workspace_bytes(0, 64) == 0
    det = lib.vn_rpn_detect_workspace_bytes(2, 70400, 1024)
    assert det >= sel + lib.vn_box_nms_workspace_bytes(2, 1024) + 2 * 1024 * (7 + 1 + 1) * 4
    assert lib.vn_rpn_detect_workspace_bytes(2, 70400, 0) == 0 and lib.vn_rpn_detect_workspace_bytes(2, 70400, 4097) == 0


def test_select_decode_checks_its_arguments():
    from voxelnet_amd import _lib
    lib = _lib.load()
    _, p = _buf()
    need = lib.vn_rpn_select_decode_workspace_bytes(1, 8, 4)

    def sel(ptr, B, N, pre, ws, ws_bytes):
        return lib.vn_rpn_select_decode(ptr, ptr, ptr, B, N, 0.5, pre, 1.56, ptr, ptr, ptr, ptr, ws, ws_bytes, None)
    assert sel(None, 1, 8, 4, p, need) == EINVAL                     # NULL pointers
    assert sel(p, 1, 8, 4, None, need) == EINVAL                     # NULL workspace
    assert sel(p, 1, 8, 0, p, 1 << 20) == EINVAL and sel(p, 1, 8, 4097, p, 1 << 20) == EINVAL
    assert sel(p, 0, 8, 4, p, 1 << 20) == EINVAL and sel(p, 1, 0, 4, p, 1 << 20) == EINVAL
    assert sel(p, 1, 8, 4, p, need - 1) == EWORKSPACE


def test_box_nms_checks_its_arguments():
    from voxelnet_amd import _lib
    lib = _lib.load()
    _, p = _buf()
    need = lib.vn_box_nms_workspace_bytes(1, 4)

    def nms(ptr, B, K, mode, thr, post, ws, ws_bytes):
        return lib.vn_box_nms(ptr, ptr, B, K, mode, thr, post, ptr, ptr, ws, ws_bytes, None)
    assert nms(None, 1, 4, 1, 0.1, 4, p, need) == EINVAL               # NULL pointers
    assert nms(p, 1, 4, 1, 0.1, 4, None, need) == EINVAL               # NULL workspace
    assert nms(p, 1, 0, 1, 0.1, 4, p, 1 << 20) == EINVAL               # K = 0
    assert nms(p, 1, 4097, 1, 0.1, 4, p, 1 << 20) == EINVAL            # K = 4097
    assert nms(p, 1, 4, 1, 0.1, 65, p, 1 << 20) == EINVAL              # post = 65
    assert nms(p, 1, 4, 1, 0.1, 0, p, 1 << 20) == EINVAL
    assert nms(p, 1, 4, 2, 0.1, 4, p, 1 << 20) == EINVAL and nms(p, 1, 4, -1, 0.1, 4, p, 1 << 20) == EINVAL
    assert nms(p, 1, 4, 0, float("nan"), 4, p, 1 << 20) == EINVAL      # a NaN threshold
    assert nms(p, 1, 4, 1, float("inf"), 4, p, 1 << 20) == EINVAL
    assert nms(p, 0, 4, 1, 0.1, 4, p, 1 << 20) == EINVAL
    assert nms(p, 1, 4, 1, 0.1, 4, p, need - 1) == EWORKSPACE
    assert nms(p, 1, 4, 0, 0.1, 4, p, 0) == EWORKSPACE


def test_detect_checks_its_arguments():
    from voxelnet_amd import _lib
    lib = _lib.load()
    _, p = _buf()
    need = lib.vn_rpn_detect_workspace_bytes(1, 8, 4)

    def det(ptr, B, N, pre, mode, thr, post, ws, ws_bytes):
        return lib.vn_rpn_detect(ptr, ptr, ptr, B, N, 0.5, pre, mode, thr, post, 1.56, ptr, ptr, ptr, ws, ws_bytes, None)
    assert det(None, 1, 8, 4, 1, 0.1, 4, p, need) == EINVAL
    assert det(p, 1, 8, 4, 1, 0.1, 4, None, need) == EINVAL
    assert det(p, 1, 8, 0, 1, 0.1, 4, p, 1 << 20) == EINVAL and det(p, 1, 8, 4097, 1, 0.1, 4, p, 1 << 20) == EINVAL
    assert det(p, 1, 8, 4, 1, 0.1, 65, p, 1 << 20) == EINVAL and det(p, 1, 8, 4, 1, 0.1, 0, p, 1 << 20) == EINVAL
    assert det(p, 1, 8, 4, 2, 0.1, 4, p, 1 << 20) == EINVAL
    assert det(p, 1, 8, 4, 0, float("nan"), 4, p, 1 << 20) == EINVAL
    assert det(p, 1, 8, 4, 1, 0.1, 4, p, need - 1) == EWORKSPACE


def test_python_surface_refuses_cpu_and_bad_arguments():
    import torch
    from voxelnet_amd import _lib
    from voxelnet_amd import predict as P
    assert P.EVAL_DECODE == dict(score_thres=0.1, nms="rotated", nms_thres=0.1, pre_nms_top_k=1024)
    with pytest.raises(_lib.VoxelnetHipError):
        P.nms_device(torch.zeros(1, 4, 7), torch.zeros(1, dtype=torch.int32))
    with pytest.raises(_lib.VoxelnetHipError):
        P.BoxDecoder("Car", "cpu")
