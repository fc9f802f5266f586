"""Host: the true-IoU target assignment's reference (tests/assign_ref.py) on its own — the properties
the rules promise, and, for every case tests/test_gpu_assign.py compares the device on, that no decision lies within the
margin (so that a last-bit difference of the device's IoUs cannot flip one).  No GPU, no library call except the
argument checks at the end (the HIP library's host code)."""
import ctypes

import numpy as np
import pytest

import assign_cases as C
import assign_ref as A

ALL = C.cases() + (C.hand_frames(),)


@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("case", ALL, ids=[c.id for c in ALL])
def test_reference_properties_and_guard(case, kind):
    gap = case.guard(kind)
    print(f"{case.id} {kind}: smallest gap {gap:.3e}")
    assert gap > C.MARGIN
    for boxes, s in zip(case.boxes, case.ref(kind)):
        assert not (s["pos"] & s["neg"]).any()                                    # exclusive
        if len(boxes) == 0:
            assert s["neg"].all() and not s["pos"].any() and (s["matched"] == -1).all()
            continue
        M = s["iou"].max(axis=0)
        for k in np.flatnonzero(M > 0):
            # a positive whose IoU with box k is M_k: matched to k, or to a copy / a better box of its own
            best = np.flatnonzero(s["iou"][:, k] == M[k])
            assert s["pos"][best].any(), k
        assert (s["matched"][s["pos"]] >= 0).all() and (s["matched"][~s["pos"]] == -1).all()
        assert (s["targets"][~s["pos"]] == 0).all()
        m = s["iou"].max(axis=1)
        assert s["pos"][m >= np.float32(case.pos_iou)].all()
        assert not s["neg"][m >= np.float32(case.neg_iou)].any()


def test_cases_contain_what_they_were_built_for():
    sizes = {c.id: c.n_anchors for c in C.cases()}
    assert [sizes[k] for k in ("Car-1x1", "Car-5x13", "Car-16x8", "Car-9x15", "Car-tiled", "Car-full")] == [2, 130, 256, 270, 810, 70400]
    by_id = {c.id: c for c in C.cases()}
    assert [len(b) for b in by_id["Car-9x15"].boxes] == [5, 0, 12] and [len(b) for b in by_id["Car-5x13-128boxes"].boxes] == [128]
    for kind in C.KINDS:
        forced = thr = 0
        for c in C.cases():
            for s in c.ref(kind):
                if s["iou"].shape[1]:
                    m = s["iou"].max(axis=1)
                    thr += int((m >= np.float32(c.pos_iou)).sum())
                    forced += int((s["pos"] & (m < np.float32(c.pos_iou))).sum())
        assert thr >= 10 and forced >= 5, (kind, thr, forced)
        # tiled: each box's best IoU is reached in all three copies of the grid, the positive sits in the FIRST
        t = by_id["Car-tiled"]
        n1 = t.n_anchors // 3
        seen = 0
        for s in t.ref(kind):
            if s["iou"].shape[1] == 0:
                continue
            m = s["iou"].max(axis=1)
            only = np.flatnonzero(s["pos"] & (m < np.float32(t.pos_iou)))
            assert (only < n1).all()
            seen += len(only)
            assert np.array_equal(s["iou"][:n1], s["iou"][n1:2 * n1])
        assert seen >= 1


def test_hand_made_frames():
    h = C.hand_frames()
    for kind in C.KINDS:
        f0, f1, f2, f3 = h.ref(kind)
        # 0: both boxes have positives, and some anchor has an IoU > 0 with both (they compete)
        assert set(f0["matched"][f0["pos"]].tolist()) == {0, 1}
        assert ((f0["iou"] > 0).sum(axis=1) == 2).any()
        # 1: one forced positive below pos_iou, not negative although its IoU may lie below neg_iou
        assert f1["pos"].sum() == 1 and f1["iou"].max() < np.float32(h.pos_iou)
        n = int(np.flatnonzero(f1["pos"])[0])
        assert n == int(f1["iou"][:, 0].argmax()) and not f1["neg"][n]
        # 2: the box outside the grid has no positive
        assert f2["iou"][:, 0].max() == 0 and set(f2["matched"][f2["pos"]].tolist()) == {1}
        # 3: w = 0
        if kind == "rotated":
            assert f3["iou"][:, 0].max() == 0 and set(f3["matched"][f3["pos"]].tolist()) == {1}
        else:
            assert f3["iou"][:, 0].max() > 0


def test_standup_equals_rotated_for_axis_aligned_boxes():
    """yaw 0 and pi/2 on both sides: the hull IS the footprint (to the rounding of cos(pi/2) = 6e-17)"""
    c = C.cases()[1]                                     # Car 5x13
    rng = np.random.default_rng(11)
    boxes = c.boxes[0].copy()
    boxes[:, 6] = rng.choice([0.0, np.pi / 2], len(boxes))
    s = A.iou_table(c.anchors, boxes, "standup")
    r = A.iou_table(c.anchors, boxes, "rotated")
    assert (r > 0).sum() > 50
    np.testing.assert_allclose(s, r, rtol=0, atol=1e-12)


def test_stand_up_plateau_ties_are_exact():
    """anchors of one row that all contain a box's hull along x have THE SAME stand-up IoU bit for bit"""
    c = C.cases()[3]
    a = c.anchors.reshape(-1, 7)
    row = a[(a[:, 1] == a[0, 1]) & (a[:, 6] == 0)]
    box = np.array([row[3, 0] + 0.13, row[0, 1] + 0.21, -1.7, 1.5, 1.6, 1.9, np.pi / 2])          # hull 1.6 wide along x
    v = [A.standup_iou(q, box) for q in row[1:6]]
    assert v[0] > 0 and len(set(v)) == 1
    assert A.same_by_construction("standup", row[1], row[5], box) and not A.same_by_construction("rotated", row[1], row[5], box)


def test_argument_checks_of_the_library():
    """host code of vn_rpn_targets_iou / vn_rpn_*_layout: every status is returned before anything is launched"""
    from voxelnet_amd import _lib
    lib = _lib.load()
    assert _lib.missing_symbols() == []
    assert (_lib.VN_ASSIGN_STANDUP, _lib.VN_ASSIGN_ROTATED, _lib.VN_DETECT_FLAT, _lib.VN_DETECT_SITE) == (1, 2, 0, 1)
    need = lib.vn_rpn_targets_iou_workspace_bytes(2, 70400, 128)
    assert need >= 2 * 70400 * 12 + 2 * 128 * 12
    assert lib.vn_rpn_targets_iou_workspace_bytes(2, 70400, 129) == 0 and lib.vn_rpn_targets_iou_workspace_bytes(0, 8, 1) == 0
    assert lib.vn_rpn_targets_iou_workspace_bytes(2, 0, 1) == 0 and lib.vn_rpn_targets_iou_workspace_bytes(2, 1 << 30, 1) == 0
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    nan = float("nan")

    def call(kind=1, pos=0.6, neg=0.45, ws=need, max_gt=128, anchors=p, matched=None, h=1.56):
        return lib.vn_rpn_targets_iou(anchors, 70400, p, p, 2, max_gt, kind, pos, neg, h, p, p, p, matched, p, ws, None)
    for bad in (dict(kind=0), dict(kind=3), dict(pos=nan), dict(neg=nan), dict(max_gt=129), dict(max_gt=0), dict(anchors=None),
                dict(h=0.0)):
        assert call(**bad) == -1, bad
    assert call(ws=need - 1) == -3
    # the layout argument: unknown value, odd anchor count with the site layout
    sel = lib.vn_rpn_select_decode_workspace_bytes(1, 9, 4)
    det = lib.vn_rpn_detect_workspace_bytes(1, 9, 4)
    assert lib.vn_rpn_select_decode_layout(p, p, p, 1, 9, 0.5, 4, 1.56, p, p, p, p, p, sel, None, 1) == -1
    assert lib.vn_rpn_select_decode_layout(p, p, p, 1, 9, 0.5, 4, 1.56, p, p, p, p, p, sel, None, 2) == -1
    assert lib.vn_rpn_select_decode_layout(p, p, p, 1, 9, 0.5, 4, 1.56, p, p, p, p, p, sel - 1, None, 0) == -3
    assert lib.vn_rpn_detect_layout(p, p, p, 1, 9, 0.5, 4, 1, 0.1, 4, 1.56, p, p, p, p, det, None, 1) == -1
    assert lib.vn_rpn_detect_layout(p, p, p, 1, 9, 0.5, 4, 1, 0.1, 4, 1.56, p, p, p, p, det, None, -1) == -1
    assert lib.vn_rpn_detect_layout(p, p, p, 1, 8, 0.5, 4, 1, 0.1, 4, 1.56, p, p, p, p, 0, None, 1) == -3
