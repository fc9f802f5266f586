"""Inputs of the true-IoU target assignment, shared by tests/test_assign_host.py — which asserts ON THE
REFERENCE ALONE (tests/assign_ref.py) that no decision of any case lies within MARGIN — and tests/test_gpu_assign.py, and
the frames of the round trip (tests/test_gpu_detect_site.py).  Anchor grids and boxes are tests/label_cases.py's."""
import functools

import numpy as np

import assign_ref as A
import label_cases as L
from oracle import targets as ot

MARGIN = 1e-7          # tests/test_gpu_detect.py's: two orders above the 1e-9 device / reference agreement of the pair function
KINDS = A.KINDS
SEED, COUNTS = L.SLICE_SEEDS[0]          # (5, (5, 0, 12)): an empty sample in the middle


class AssignCase:
    def __init__(self, name, cls_name, anchors, boxes):
        self.id, self.cls_name, self.anchors, self.boxes = name, cls_name, anchors, boxes
        self.shape = tuple(anchors.shape[:2])
        self.n_anchors = anchors.shape[0] * anchors.shape[1] * 2
        c = ot.CLASSES[cls_name]
        self.pos_iou, self.neg_iou, self.anchor_h = c["pos"], c["neg"], c["h"]

    @functools.lru_cache(maxsize=None)
    def ref(self, kind):
        """the reference's answer per sample (computed once, read-only)"""
        out = A.assign(self.anchors, self.boxes, kind, self.pos_iou, self.neg_iou, self.anchor_h)
        for s in out:
            for v in s.values():
                v.setflags(write=False)
        return out

    def guard(self, kind):
        """asserts the guard on the reference alone -> the smallest gap over the samples"""
        return min(A.guard(self.anchors, b, s["iou"], self.pos_iou, self.neg_iou, MARGIN, kind)
                   for b, s in zip(self.boxes, self.ref(kind)))


def _from_label_case(name, cls_name, grid, seed=SEED, counts=COUNTS):
    c = L.target_case(cls_name, grid, seed, counts)
    return AssignCase(name, cls_name, c.anchors, c.boxes)


@functools.lru_cache(maxsize=None)
def cases():
    out = [_from_label_case("Car-%dx%d" % hw, "Car", hw) for hw in ((1, 1), (5, 13), (16, 8), (9, 15))]
    out.append(_from_label_case("Car-tiled", "Car", "tiled"))
    # 128 boxes on 130 anchors: seeds 1 and 8 hold the guard in both kinds; under 2, 4, 6, 7, 9 and 10 a box at the slice's edge
    # has two crossing anchors (the anchor's short side inside the box's long side: sliding it along the box does not change
    # the intersection) as its best ones, an exact tie mathematically that rounding breaks
    out.append(_from_label_case("Car-5x13-128boxes", "Car", (5, 13), 1, (128,)))
    out.append(_from_label_case("Car-full", "Car", "full"))
    out.append(_from_label_case("Pedestrian-9x15", "Pedestrian", (9, 15)))
    return tuple(out)


def hand_frames():
    """-> AssignCase on the Car slice anchors[100:124, 60:92] (N = 1536) with one sample per hand-made frame:
    0  two overlapping boxes that compete for the anchors between them
    1  a box at 45 degrees: its best anchor stays below pos_iou in both kinds — the forced positive, which is not negative
    2  a box outside the grid (M_k = 0: no positive) next to one inside
    3  a box with w = 0 next to a normal one: rotated IoU 0 (the stand-up hull of a segment still has an extent)"""
    anchors = np.ascontiguousarray(ot.generate_anchors("Car")[100:124, 60:92])
    a = anchors.reshape(-1, 7)
    x0, x1, y0, y1 = a[:, 0].min(), a[:, 0].max(), a[:, 1].min(), a[:, 1].max()

    def car(fx, fy, r, **kw):
        q = [x0 + fx * (x1 - x0), y0 + fy * (y1 - y0), -1.7, 1.5, 1.65, 4.0, r]
        for k, v in kw.items():
            q[int(k[1:])] = v
        return q
    # (fractions that put no box midway between two rows or columns of anchors: a symmetric pair of anchors ties)
    frames = [[car(0.41, 0.53, 0.05), car(0.41, 0.53, 0.05, f0=x0 + 0.41 * (x1 - x0) + 0.7, f1=y0 + 0.53 * (y1 - y0) + 0.3)],
              [car(0.53, 0.47, 0.785)],
              [car(0.3, 0.3, 0.2, f0=x1 + 30.0), car(0.71, 0.62, -1.3)],
              [car(0.31, 0.43, 0.3, f4=0.0), car(0.71, 0.62, 0.1)]]
    return AssignCase("Car-hand", "Car", anchors, [np.array(f, dtype=np.float64).reshape(-1, 7) for f in frames])


# ---- the round trip (tests/test_gpu_detect_site.py): frames of well-separated cars as KITTI label lines
ROUND_TRIP_FRACTIONS = (((0.25, 0.3), (0.75, 0.7)), ((0.5, 0.5),), ())
ROUND_TRIP_YAWS = (0.2, -1.3, 0.8)


def round_trip_frames(anchors):
    """-> label lines per frame: cars at ROUND_TRIP_FRACTIONS of the extent of the anchors' centres, yaws ROUND_TRIP_YAWS in
    turn, sizes inside eval_ref._SCENE["Car"]'s ranges, default difficulty fields (valid at every difficulty)"""
    import eval_ref as R
    a = np.asarray(anchors).reshape(-1, 7)
    x0, x1, y0, y1 = a[:, 0].min(), a[:, 0].max(), a[:, 1].min(), a[:, 1].max()
    sizes = ((1.5, 1.6, 3.9), (1.6, 1.7, 4.2), (1.45, 1.55, 3.6))          # (h, w, l)
    frames, i = [], 0
    for fr in ROUND_TRIP_FRACTIONS:
        lines = []
        for fx, fy in fr:
            h, w, l = sizes[i % 3]
            lines.append(R.label_line("Car", [x0 + fx * (x1 - x0), y0 + fy * (y1 - y0), -1.7, h, w, l, ROUND_TRIP_YAWS[i % 3]]))
            i += 1
        frames.append(lines)
    return frames
