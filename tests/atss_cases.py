"""Inputs of the ATSS target assignment, shared by tests/test_atss_host.py — which asserts ON THE
REFERENCE ALONE (tests/atss_ref.py) that no decision of any (case, kind, top_k) lies within MARGIN — and
tests/test_gpu_atss.py.  The anchor grids and boxes are tests/assign_cases.py's (its cases and hand-made frames), plus frames
of this file's own on the same Car slice."""
import functools

import numpy as np

import assign_cases as C
import atss_ref as T

MARGIN = C.MARGIN
KINDS = T.KINDS
TOP_KS = (1, 9, 32)          # the smallest, the published default, VN_ATSS_MAX_TOPK (above the 1x1 grid's one site per group)


class AtssCase:
    """an assign_cases.AssignCase's anchors and boxes with the ATSS reference's answers, computed once and read-only"""

    def __init__(self, base):
        self.base, self.id, self.cls_name = base, base.id, base.cls_name
        self.anchors, self.boxes, self.shape, self.n_anchors, self.anchor_h = base.anchors, base.boxes, base.shape, base.n_anchors, base.anchor_h

    @functools.lru_cache(maxsize=None)
    def _order(self):
        """per sample, per box: the two groups' anchors ranked by (d2, n) (None for an invalid box) — shared by every
        (kind, top_k); only the head of each ranking is kept"""
        return [[[grp[:33] for grp in T.ranked(self.anchors, q)[0]] if T.box_valid(q) else None for q in b] for b in self.boxes]

    @functools.lru_cache(maxsize=None)
    def ref(self, kind, top_k):
        out = [T.assign_sample(self.anchors, b, kind, top_k, self.anchor_h, order=o) for b, o in zip(self.boxes, self._order())]
        for s in out:
            for v in s.values():
                for x in (v if isinstance(v, list) else [v]):
                    x.setflags(write=False)
        return out

    @functools.lru_cache(maxsize=None)
    def guard(self, kind, top_k):
        """asserts the guard on the reference alone -> the smallest gap of each sort over the samples"""
        gaps = [T.guard(self.anchors, b, s, top_k, MARGIN) for b, s in zip(self.boxes, self.ref(kind, top_k))]
        return {key: min(g[key] for g in gaps) for key in gaps[0]}


def extra_frames():
    """-> AssignCase on assign_cases.hand_frames()'s Car slice (N = 1536), one sample per frame:
    0  two copies of one box: the smaller k takes every anchor
    1  no box at all, between two samples that have some
    2  a box with w = 0 (invalid: no candidates, stats of zeros) beside a valid one
    3  a box 30 m off the grid: it has candidates, every IoU is 0, no positive, stats (0, 0, 0, 0)"""
    h = C.hand_frames()
    a = h.anchors.reshape(-1, 7)
    x0, x1, y0, y1 = a[:, 0].min(), a[:, 0].max(), a[:, 1].min(), a[:, 1].max()

    def car(fx, fy, r, w=1.65, dx=0.0):
        return [x0 + fx * (x1 - x0) + dx, y0 + fy * (y1 - y0), -1.7, 1.5, w, 4.0, r]
    frames = [[car(0.37, 0.58, 0.15), car(0.37, 0.58, 0.15)],
              [],
              [car(0.31, 0.43, 0.3, w=0.0), car(0.71, 0.62, 0.1)],
              [car(0.3, 0.3, 0.2, dx=(x1 - x0) + 30.0)]]
    return C.AssignCase("Car-atss-extra", "Car", h.anchors, [np.array(f, dtype=np.float64).reshape(-1, 7) for f in frames])


def one_box_small_grid():
    """a 4 x 7 slice of the Car grid (28 sites per group <= 32) with one box: at top_k = 32 every anchor is a candidate"""
    from oracle import targets as ot
    anchors = np.ascontiguousarray(ot.generate_anchors("Car")[100:104, 60:67])
    a = anchors.reshape(-1, 7)
    q = [a[:, 0].min() + 0.43 * np.ptp(a[:, 0]), a[:, 1].min() + 0.57 * np.ptp(a[:, 1]), -1.7, 1.5, 1.65, 4.0, 0.35]
    return C.AssignCase("Car-4x7-one-box", "Car", anchors, [np.array([q], dtype=np.float64)])


@functools.lru_cache(maxsize=None)
def cases():
    return tuple(AtssCase(c) for c in C.cases() + (C.hand_frames(), extra_frames(), one_box_small_grid()))


def combos():
    """every (case, kind, top_k) the GPU test runs"""
    return [(c, kind, k) for c in cases() for kind in KINDS for k in TOP_KS]


def combo_id(combo):
    return "%s-%s-k%d" % (combo[0].id, combo[1], combo[2])
