"""CPU: the detection-scoring protocol's host side — the float64 reference tests/eval_ref.py against
closed forms, evaluate.gt_flags_from_labels on hand-written label lines, the AP arithmetic (evaluate.average_precision and
the reference's) on hand-made status lists, and the argument checks of the two new entry points (status codes, no GPU)."""
import ctypes
import math

import numpy as np
import pytest

import eval_ref as R

TOL = 1e-12


def _both(a, b):
    return R.iou_pair(np.array(a, dtype=np.float64), np.array(b, dtype=np.float64))


BOX = [20.0, -3.0, -1.5, 1.6, 1.7, 4.2, 0.4]          # x y z h w l r


def test_reference_identical_boxes():
    bev, v3 = _both(BOX, BOX)
    assert abs(bev - 1) <= TOL and abs(v3 - 1) <= TOL


def test_reference_disjoint_and_edge_touching():
    far = list(BOX)
    far[0] += 30
    assert _both(BOX, far) == (0.0, 0.0)
    a = [10.0, 2.0, -1.0, 1.5, 2.0, 4.0, 0.0]
    b = [14.0, 2.0, -1.0, 1.5, 2.0, 4.0, 0.0]          # shares the edge x = 12
    bev, v3 = _both(a, b)
    assert abs(bev) <= TOL and abs(v3) <= TOL
    c = [10.0, 2.0, 0.5, 1.5, 2.0, 4.0, 0.0]           # same footprint, stacked on top: BEV 1, 3D 0
    bev, v3 = _both(a, c)
    assert abs(bev - 1) <= TOL and v3 == 0.0


def test_reference_twin_with_w_l_swapped_and_quarter_turn():
    x, y, z, h, w, l, r = BOX
    bev, v3 = _both(BOX, [x, y, z, h, l, w, r + math.pi / 2])
    assert abs(bev - 1) <= TOL and abs(v3 - 1) <= TOL


def test_reference_copy_shifted_by_half_a_length_along_its_heading():
    x, y, z, h, w, l, r = BOX
    moved = [x + l / 2 * math.cos(r), y + l / 2 * math.sin(r), z, h, w, l, r]
    bev, v3 = _both(BOX, moved)          # I = w*l/2, union = 3/2 w*l
    assert abs(bev - 1 / 3) <= TOL and abs(v3 - 1 / 3) <= TOL


def test_reference_box_containing_another():
    big = [30.0, 5.0, -2.0, 2.0, 6.0, 9.0, 0.3]
    small = [30.4, 5.2, -1.8, 1.0, 1.5, 3.0, -0.9]
    bev, v3 = _both(big, small)
    assert abs(bev - (1.5 * 3.0) / (6.0 * 9.0)) <= TOL
    assert abs(v3 - (1.0 * 1.5 * 3.0) / (2.0 * 6.0 * 9.0)) <= TOL
    assert abs(_both(small, big)[0] - bev) <= TOL


@pytest.mark.parametrize("ra,rb", [(0.0, 0.0), (0.0, math.pi / 2), (math.pi / 2, math.pi / 2), (math.pi / 2, 0.0)])
def test_reference_axis_aligned_pairs_against_the_rectangle_formula(ra, rb):
    rng = np.random.default_rng(5)
    for _ in range(20):
        a = [rng.uniform(10, 60), rng.uniform(-30, 30), -1.5, 1.5, rng.uniform(1.5, 2), rng.uniform(3, 5), ra]
        b = [a[0] + rng.uniform(-3, 3), a[1] + rng.uniform(-3, 3), -1.2, 1.6, rng.uniform(1.5, 2), rng.uniform(3, 5), rb]

        def rect(q):          # (x extent, y extent) half sizes: r = 0 -> l along x; r = pi/2 -> l along y
            return (q[5] / 2, q[4] / 2) if q[6] == 0.0 else (q[4] / 2, q[5] / 2)
        (ax, ay), (bx, by) = rect(a), rect(b)
        ix = max(0.0, min(a[0] + ax, b[0] + bx) - max(a[0] - ax, b[0] - bx))
        iy = max(0.0, min(a[1] + ay, b[1] + by) - max(a[1] - ay, b[1] - by))
        inter = ix * iy
        want = inter / (a[4] * a[5] + b[4] * b[5] - inter)
        assert abs(_both(a, b)[0] - want) <= TOL


def test_reference_3d_with_half_vertical_overlap():
    x, y, z, h, w, l, r = BOX
    bev, v3 = _both(BOX, [x, y, z + h / 2, h, w, l, r])          # I3 = w*l*h/2, union = 3/2 h*w*l
    assert abs(bev - 1) <= TOL and abs(v3 - 1 / 3) <= TOL


def test_reference_degenerate_boxes_score_zero():
    for k, v in ((4, 0.0), (5, -1.0), (3, 0.0), (0, float("nan")), (6, float("inf"))):
        bad = list(BOX)
        bad[k] = v
        assert _both(BOX, bad) == (0.0, 0.0) and _both(bad, BOX) == (0.0, 0.0)


def test_reference_operand_order():
    scene = R.make_scene(11, n_frames=8)
    worst = 0.0
    for boxes, _, lines in scene:
        gt, _ = R.frame_ground_truth(lines)
        for d in boxes.astype(np.float64):
            for g in gt:
                for u, v in zip(R.iou_pair(d, g), R.iou_pair(g, d)):
                    worst = max(worst, abs(u - v))
    assert worst <= 1e-14, worst


# type trunc occ alpha x1 y1 x2 y2 h w l x y z ry
LINES = [
    "Car 0.00 0 1.55 300.00 150.00 400.00 200.00 1.50 1.60 3.90 1.00 1.60 20.00 -1.57",          # every difficulty
    "Car 0.20 1 1.55 300.00 150.00 400.00 180.00 1.50 1.60 3.90 -4.00 1.60 25.00 -1.20",         # moderate, hard
    "Car 0.40 2 1.55 300.00 150.00 400.00 176.00 1.50 1.60 3.90 6.00 1.60 30.00 0.30",           # hard only
    "Car 0.00 0 1.55 300.00 150.00 400.00 170.00 1.50 1.60 3.90 9.00 1.60 40.00 0.00",           # 20 px high: none but "all"
    "Pedestrian 0.00 0 0.20 500.00 150.00 520.00 210.00 1.70 0.60 0.80 3.00 1.50 12.00 0.10",    # dropped
    "Van 0.00 0 1.55 300.00 150.00 400.00 220.00 2.10 1.90 5.20 -8.00 1.70 35.00 -1.60",         # ignored everywhere
    "DontCare -1 -1 -10 503.89 169.71 590.61 190.13 -1 -1 -1 -1000 -1000 -1000 -10",            # dropped
]


def test_gt_flags_from_labels_on_hand_written_lines():
    from voxelnet_amd.evaluate import gt_flags_from_labels
    from voxelnet_amd.targets import label_to_gt_box_3d
    boxes, flags, n_valid = gt_flags_from_labels([LINES, [], LINES[4:]], "Car", ("all", "easy", "moderate", "hard"))
    assert [b.shape for b in boxes] == [(5, 7), (0, 7), (1, 7)] and all(b.dtype == np.float64 for b in boxes)
    assert np.array_equal(boxes[0], label_to_gt_box_3d([LINES], "Car", "lidar")[0])          # Car + Van lines, label order
    assert flags[0].dtype == np.uint8
    assert flags[0].tolist() == [[0, 0, 0, 0, 1], [0, 1, 1, 1, 1], [0, 0, 1, 1, 1], [0, 0, 0, 1, 1]]
    assert flags[1].shape == (4, 0) and flags[2].tolist() == [[1], [1], [1], [1]]
    assert n_valid.tolist() == [[4, 1, 2, 3], [0, 0, 0, 0], [0, 0, 0, 0]]
    # the reference's restatement agrees
    rb, rf = R.frame_ground_truth(LINES, "Car")
    assert np.array_equal(rb, boxes[0]) and np.array_equal(rf.astype(np.uint8), flags[0])
    # another class, another subset of difficulties
    pb, pf, pn = gt_flags_from_labels([LINES], "Pedestrian", ("hard", "all"))
    assert pb[0].shape == (1, 7) and pf[0].tolist() == [[0], [0]] and pn.tolist() == [[1, 1]]


def _aps(scores, status, n, points):
    from voxelnet_amd.evaluate import average_precision
    got, ref = average_precision(scores, status, n, points), R.average_precision(scores, status, n, points)
    assert (math.isnan(got) and math.isnan(ref)) or abs(got - ref) <= TOL
    return got


def test_average_precision_on_hand_made_lists():
    # 4 valid ground truths; pooled in (frame, index) order, scores out of order on purpose.  By score: TP .95, FP .90,
    # TP .85, IGNORED .80 (dropped), TP .70  ->  precision 1, 1/2, 2/3, 3/4 at recall 1/4, 1/4, 2/4, 3/4.
    # p_interp(r) = 1 for r <= 1/4, 3/4 for 1/4 < r <= 3/4, 0 above.
    scores = [0.85, 0.95, 0.70, 0.90, 0.80]
    status = [1, 1, 1, 0, -1]
    # R40: r = k/40; k = 1..10 -> 1, k = 11..30 -> 3/4, k = 31..40 -> 0:  (10 + 20 * 0.75) / 40 = 0.625
    assert abs(_aps(scores, status, 4, 40) - 0.625) <= TOL
    # R11: r = 0, .1, .2 -> 1;  .3 .. .7 -> 3/4 (5 points);  .8, .9, 1 -> 0:  (3 + 3.75) / 11
    assert abs(_aps(scores, status, 4, 11) - 6.75 / 11) <= TOL
    # equal scores keep their (frame, index) order: FP then TP -> precision 0, 1/2 at recall 0, 1 -> p_interp = 1/2 for
    # every r > 0 (R40 = 1/2; R11 the same, r = 0 included: the best precision at a recall >= 0 is 1/2)
    assert abs(_aps([0.9, 0.9], [0, 1], 1, 40) - 0.5) <= TOL
    assert abs(_aps([0.9, 0.9], [0, 1], 1, 11) - 0.5) <= TOL
    assert abs(_aps([0.9, 0.9], [1, 0], 1, 40) - 1.0) <= TOL
    # no valid ground truth: NaN, reported as such; ground truths but no detection (or only ignored ones): 0
    assert math.isnan(_aps([0.9], [0], 0, 40))
    assert _aps([], [], 3, 40) == 0.0 and _aps([0.99], [-1], 3, 11) == 0.0
    # all found, no false positive: 1
    assert abs(_aps([0.99, 0.98, 0.97], [1, 1, 1], 3, 40) - 1.0) <= TOL


def test_generator_makes_the_four_difficulties_differ():
    ev = R.RefEvaluator()
    for boxes, scores, lines in R.make_scene(0, n_frames=16):
        assert boxes.dtype == np.float32 and scores.dtype == np.float32 and boxes.shape[0] <= 20
        assert ((scores >= np.float32(0.96)) & (scores < 1)).all()
        ev.add_frame(boxes, scores, lines)
    n = ev.compute()["n_gt"]
    assert len({n[d] for d in R.DIFFS}) == 4 and n["all"] > n["hard"] > n["moderate"] > n["easy"] > 0, n


def test_new_entry_points_check_their_arguments():
    from voxelnet_amd import _lib
    lib = _lib.load()
    EINVAL = -1
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    # vn_box_iou_rotated
    assert lib.vn_box_iou_rotated(None, 1, None, 1, 0, None, None) == EINVAL
    assert lib.vn_box_iou_rotated(p, 1, p, 1, 2, p, None) == EINVAL          # metric 2
    assert lib.vn_box_iou_rotated(None, 0, None, 5, 2, None, None) == EINVAL
    assert lib.vn_box_iou_rotated(None, -1, None, 5, 0, None, None) == EINVAL
    assert lib.vn_box_iou_rotated(None, 0, None, 5, 1, None, None) == 0      # nothing to do
    # vn_eval_match
    need = lib.vn_eval_match_workspace_bytes(2, 20, 128)
    assert need >= 2 * 20 * 4
    assert lib.vn_eval_match_workspace_bytes(2, 33, 128) == 0 and lib.vn_eval_match_workspace_bytes(2, 20, 129) == 0

    def match(ptr, B, top_k, max_gt, n_diff, ws, ws_bytes, thr=0.7):
        return lib.vn_eval_match(ptr, ptr, ptr, ptr, ptr, ptr, B, top_k, max_gt, n_diff, thr, thr, ptr, ptr, None, ws, ws_bytes, None)
    assert match(None, 2, 20, 128, 4, None, 0) == EINVAL                      # NULL pointers
    assert match(p, 2, 20, 128, 4, None, need) == EINVAL                      # NULL workspace
    assert match(p, 2, 33, 128, 4, p, 1 << 20) == EINVAL                      # top_k 33
    assert match(p, 2, 20, 129, 4, p, 1 << 20) == EINVAL                      # max_gt 129
    assert match(p, 2, 20, 128, 0, p, 1 << 20) == EINVAL and match(p, 2, 20, 128, 9, p, 1 << 20) == EINVAL
    assert match(p, 2, 20, 128, 4, p, need - 1) == EINVAL                     # a too-small workspace
    assert match(p, 2, 20, 128, 4, p, 1 << 20, thr=float("nan")) == EINVAL
    assert match(None, 0, 20, 128, 4, None, 0) == 0                           # B = 0: nothing to do
    assert match(None, 0, 33, 128, 4, None, 0) == EINVAL


def test_evaluator_refuses_cpu():
    import torch
    from voxelnet_amd import _lib
    from voxelnet_amd import evaluate as E
    with pytest.raises(_lib.VoxelnetHipError):
        E.box_iou_rotated(torch.zeros(1, 7, dtype=torch.float64), torch.zeros(1, 7, dtype=torch.float64))
    with pytest.raises(_lib.VoxelnetHipError):
        E.DetectionEvaluator("Car", device="cpu")
