"""CPU: test-time augmentation and box voting without a GPU — the reference tests/tta_ref.py against
closed forms, the host-side argument checks of vn_pool_merge / vn_box_vote (status codes, before any launch), and the Python
layer's argument checks."""
import ctypes
import inspect
import math

import numpy as np
import pytest
import torch

import tta_ref as T

EINVAL = -1


# ------------------------------------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("fy, angle, factor", [(1.0, 0.0, 1.0), (-1.0, 0.0, 1.0), (1.0, math.pi / 8, 1.05), (-1.0, -0.7, 0.95),
                                               (-1.0, 2.9, float(np.float32(1.05)))])
def test_reference_inverse_undoes_the_draws_box_rules(fy, angle, factor):
    rng = np.random.default_rng(7)
    for _ in range(20):
        box = np.array([rng.uniform(0, 70), rng.uniform(-40, 40), rng.uniform(-2, 0), 1.5, 1.6, 3.9, rng.uniform(-math.pi, math.pi)])
        back = T.inverse_box(T.forward_box(box, fy, angle, factor), fy, angle, factor)
        assert np.abs(back - box).max() <= 1e-12 * max(1.0, np.abs(box).max())


def test_reference_forward_is_the_packages_draw():
    """forward_box restates augment.draw_compose's stages 2-4 on a label box: the two agree on a drawn recipe"""
    from voxelnet_amd import augment as A
    from voxelnet_amd.synth import synth_labels
    labels = synth_labels("Car", 4, 3)
    np.random.seed(11)
    prm = A.draw_compose(labels, A.ComposeRecipe(object_rot=None, object_sigma=None, attempts=None, flip=1.0, rotation=0.6,
                                                 scale=(0.9, 1.1), translate_sigma=None))
    assert prm.flip_y and prm.has_box.sum() >= 3
    for before, after in zip(prm.boxes_before[prm.has_box], prm.boxes_after[prm.has_box]):
        assert np.allclose(T.forward_box(before, -1.0, prm.angle, prm.factor), after, rtol=0, atol=1e-12)


def _cluster(offsets, yaws, scores):
    base = np.array([20.0, 3.0, -1.0, 1.5, 1.6, 3.9, 0.3])
    rows = []
    for (dx, dy), r in zip(offsets, yaws):
        q = base.copy()
        q[0], q[1], q[6] = q[0] + dx, q[1] + dy, r
        rows.append(q)
    return np.array(rows, dtype=np.float32), np.array(scores, dtype=np.float32)


def test_reference_three_equal_members_vote_to_their_mean():
    boxes, scores = _cluster([(0.0, 0.0), (0.25, 0.0), (0.0, 0.125)], [0.25, 0.25, 0.25], [0.5, 0.5, 0.5])
    out = T.vote(boxes, scores, 3, [0], 0.5, T.W_SCORE, T.S_KEEP)
    assert out["members"].tolist() == [3] and out["t"].tolist() == [0]
    assert np.allclose(out["boxes"][0], boxes.astype(np.float64).mean(axis=0), rtol=0, atol=1e-12)
    assert out["scores"][0] == np.float32(0.5)
    # a far row is no member; a threshold above 1 leaves the kept row alone
    far = np.concatenate([boxes, boxes[:1] + np.float32([30, 0, 0, 0, 0, 0, 0])])
    out = T.vote(far, np.append(scores, np.float32(0.9)), 4, [0, 3], 0.5, T.W_SCORE, T.S_KEEP)
    assert out["members"].tolist() == [1, 3] and out["t"].tolist() == [1, 0]          # descending output score
    out = T.vote(boxes, scores, 3, [0], 2.0)
    assert out["members"].tolist() == [1] and np.array_equal(out["boxes"][0].astype(np.float32), boxes[0])


def test_reference_a_member_turned_by_pi_leaves_the_yaw_alone():
    r = 0.25
    boxes, scores = _cluster([(0.0, 0.0), (0.0, 0.0)], [r, r + math.pi], [0.75, 0.5])
    out = T.vote(boxes, scores, 2, [0], 0.5, T.W_SCORE_IOU, T.S_KEEP)
    assert out["members"].tolist() == [2]
    # the members differ by pi up to the float32 rounding of r + pi: d is that rounding, ~1e-7, not pi
    assert abs(out["boxes"][0][6] - float(boxes[0, 6])) < 2e-7
    assert out["wrap_gap"] > 1.5


def test_reference_view_mean_of_a_cluster_seen_by_two_of_four_views():
    boxes, scores = _cluster([(0.0, 0.0), (0.125, 0.0), (0.0, 0.125), (0.125, 0.125)], [0.25] * 4, [0.875, 0.5, 0.75, 0.625])
    src = np.array([0 * 10 + 0, 0 * 10 + 1, 2 * 10 + 0, 2 * 10 + 3])          # views 0, 0, 2, 2 at 10 rows per view
    out = T.vote(boxes, scores, 4, [0], 0.5, T.W_SCORE, T.S_VIEW_MEAN, src=src, rows_per_view=10, V=4)
    assert out["members"].tolist() == [4]
    assert out["scores"][0] == np.float32((0.875 + 0.75) / 4)


def test_reference_merge_order_ties_zeros_and_nan():
    boxes = np.arange(2 * 4 * 7, dtype=np.float32).reshape(2, 4, 7)
    scores = np.array([[0.5, 0.0, np.nan, 0.25], [0.5, -0.0, 0.75, 9.0]], dtype=np.float32)
    ob, os_, src = T.merge(boxes, scores, [4, 3], [(1.0, 0.0, 1.0), (1.0, 0.0, 1.0)])
    assert src.tolist() == [6, 0, 4, 3, 1, 5]          # 0.75 | 0.5 (view 0 first) 0.5 | 0.25 | +0.0 (src 1) -0.0 (src 5)
    assert np.array_equal(ob, boxes.reshape(8, 7)[src]) and np.array_equal(os_.view(np.uint32), scores.reshape(8)[src].view(np.uint32))


# ------------------------------------------------------------------------------------------- the C ABI's checks
def _buf(n=64):
    return ctypes.cast(ctypes.create_string_buffer(n), ctypes.c_void_p)


def _views(*rows):
    return np.ascontiguousarray(np.array(rows, dtype=np.float64).reshape(-1, 3))


def test_pool_merge_refuses_every_limit_before_any_launch():
    from voxelnet_amd import _lib
    lib = _lib.load()
    q = lib.vn_pool_merge_workspace_bytes
    assert q(1, 1, 1) > 0 and q(8, 1, 512) > 0 and q(4, 2, 1024) > 0
    for V, B, K in [(0, 1, 1), (9, 1, 1), (1, 0, 1), (1, 1, 0), (4, 1, 1025), (8, 1, 513), (1, 1, 4097), (-1, 1, 1), (1, -1, 1), (1, 1, -1)]:
        assert q(V, B, K) == 0, (V, B, K)
    p = _buf()          # host memory: every call below must return before it would touch it on the device
    ident = _views((1.0, 0.0, 1.0), (1.0, 0.0, 1.0), (1.0, 0.0, 1.0), (1.0, 0.0, 1.0), (1.0, 0.0, 1.0), (1.0, 0.0, 1.0),
                   (1.0, 0.0, 1.0), (1.0, 0.0, 1.0), (1.0, 0.0, 1.0))

    def call(V, B, K, views=ident, null=None):
        a = [p, p, p, ctypes.c_void_p(views.ctypes.data), V, B, K, p, p, p, p, p, 4096, None]
        if null is not None:
            a[null] = None
        return lib.vn_pool_merge(*a)
    for V, B, K in [(0, 1, 1), (9, 1, 1), (1, 0, 1), (1, 1, 0), (4, 1, 1025), (8, 1, 513), (1, 1, 4097)]:
        assert call(V, B, K) == EINVAL, (V, B, K)
    for bad in [(0.0, 0.0, 1.0), (2.0, 0.0, 1.0), (math.nan, 0.0, 1.0), (1.0, math.inf, 1.0), (1.0, math.nan, 1.0), (1.0, 0.0, 0.0),
                (1.0, 0.0, -1.0), (1.0, 0.0, math.inf), (1.0, 0.0, math.nan)]:
        assert call(2, 1, 4, _views((1.0, 0.0, 1.0), bad)) == EINVAL, bad
    for null in (0, 1, 2, 3, 7, 8, 9, 10, 11):
        assert call(1, 1, 4, null=null) == EINVAL, null
    assert lib.vn_pool_merge(None, None, None, None, 1, 1, 1, None, None, None, None, None, 0, None) == EINVAL


def test_box_vote_refuses_every_limit_before_any_launch():
    from voxelnet_amd import _lib
    lib = _lib.load()
    q = lib.vn_box_vote_workspace_bytes
    assert q(1, 1, 1, 1) > 0 and q(3, 4096, 64, 8) > 0
    for B, K, P, V in [(0, 1, 1, 1), (1, 0, 1, 1), (1, 4097, 1, 1), (1, 1, 0, 1), (1, 1, 65, 1), (1, 1, 1, 0), (1, 1, 1, 9)]:
        assert q(B, K, P, V) == 0, (B, K, P, V)
    p = _buf()

    def call(B=1, K=8, P=4, V=1, src=None, rpv=0, thres=0.5, wm=0, sm=0, null=None):
        a = [p, p, p, src, rpv, p, p, B, K, P, V, thres, wm, sm, p, p, p, p, p, 1 << 20, None]
        if null is not None:
            a[null] = None
        return lib.vn_box_vote(*a)
    for kw in [dict(B=0), dict(K=0), dict(K=4097), dict(P=0), dict(P=65), dict(V=0), dict(V=9, src=p, rpv=1), dict(thres=0.0),
               dict(thres=-0.5), dict(thres=math.inf), dict(thres=math.nan), dict(wm=2), dict(wm=-1), dict(sm=2), dict(sm=-1),
               dict(V=2), dict(V=2, src=p, rpv=0), dict(src=p, rpv=0), dict(src=p, rpv=-3)]:
        assert call(**kw) == EINVAL, kw
    for null in (0, 1, 2, 5, 6, 14, 15, 16, 17, 18):
        assert call(null=null) == EINVAL, null
    assert lib.vn_box_vote(None, None, None, None, 0, None, None, 1, 1, 1, 1, 0.5, 0, 0, None, None, None, None, None, 0, None) == EINVAL
    assert lib.vn_abi_version() == 4


# ------------------------------------------------------------------------------------------- the Python layer
def test_view_and_vote_objects_check_their_arguments():
    import dataclasses

    from voxelnet_amd import tta
    assert tta.View() == tta.View(False, 0.0, 1.0) and tta.View().identity and not tta.View(flip_y=True).identity
    assert tta.View().row() == (1.0, 0.0, 1.0) and tta.View(True, 0.5, 1.05).row() == (-1.0, 0.5, float(np.float32(1.05)))
    with pytest.raises(dataclasses.FrozenInstanceError):
        tta.View().angle = 1.0
    for kw in [dict(angle=math.inf), dict(angle=math.nan), dict(scale=0.0), dict(scale=-1.0), dict(scale=math.inf), dict(flip_y=1)]:
        with pytest.raises(ValueError):
            tta.View(**kw)
    assert tta.BoxVote() == tta.BoxVote(0.5, "score_iou", "keep")
    for kw in [dict(thres=0.0), dict(thres=-1.0), dict(thres=math.nan), dict(weight="iou"), dict(score="max")]:
        with pytest.raises(ValueError):
            tta.BoxVote(**kw)
    t = tta.TestTimeAugment()
    assert t.views == (tta.View(), tta.View(flip_y=True)) and t.vote == tta.BoxVote(score="view_mean") and t.fov_calib_dir is None
    for kw in [dict(views=()), dict(views=(tta.View(),) * 9), dict(views=((1.0, 0.0, 1.0),)), dict(vote="score")]:
        with pytest.raises(ValueError):
            tta.TestTimeAugment(**kw)


def test_cpu_tensors_raise_and_ranges_are_checked():
    from voxelnet_amd import _lib, tta
    b, s, c = torch.zeros((2, 1, 4, 7)), torch.zeros((2, 1, 4)), torch.zeros((2, 1), dtype=torch.int32)
    with pytest.raises(_lib.VoxelnetHipError):
        tta.merge_pools(b, s, c, (tta.View(), tta.View(flip_y=True)))
    with pytest.raises(_lib.VoxelnetHipError):
        tta.merge_pools([b[0], b[1]], [s[0], s[1]], [c[0], c[1]], (tta.View(), tta.View(flip_y=True)))
    k, kc = torch.zeros((1, 3), dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
    with pytest.raises(_lib.VoxelnetHipError):
        tta.vote_device(b[0], s[0], c[0], k, kc, tta.BoxVote())
    with pytest.raises(ValueError):
        tta.vote_device(b[0], s[0], c[0], k, kc, "score")
    with pytest.raises(ValueError):
        tta._view_rows([(0.5, 0.0, 1.0)])
    with pytest.raises(ValueError):
        tta._view_rows([tta.View()] * 9)
    with pytest.raises(ValueError):
        tta._view_rows([(1.0, math.nan, 1.0)])


def test_decode_and_evaluate_signatures_take_the_new_keywords():
    from voxelnet_amd import model as M
    from voxelnet_amd.predict import BoxDecoder
    for fn in (BoxDecoder.decode_device, BoxDecoder.__call__):
        assert inspect.signature(fn).parameters["vote"].default is None
    for fn in (M.RPN3D.evaluate, M.RPN3D.predict):
        assert inspect.signature(fn).parameters["tta"].default is None
    # and they still bind the calls of before
    inspect.signature(BoxDecoder.decode_device).bind(None, "p", "d", 0.5, 0.1, 20, "rotated", 1024, "site", None, 0.7, None, None, 0.5)
    inspect.signature(M.RPN3D.evaluate).bind(None, [], "cuda:0", None, None, None, None, None)
