"""Seeded inputs for the label side of the step off the Car anchor grid: ground-truth boxes, anchor grids (full, sliced,
tiled) and clustered candidate maps for the three classes, shared by tests/test_label_cases_host.py (which asserts ON THE
ORACLE ALONE that every case contains what it was built for) and by the GPU tests of csrc/targets.hip, csrc/predict.hip
and csrc/detect.hip.

The oracle for Pedestrian and Cyclist is the Car-pinned code (oracle/targets.py, oracle/predict.py: pinned to the imported
reference by tests/golden/targets_car.npz and predict_car.npz) with the other classes' constants; there is no golden of
their own.

Why the cases look as they do.  The anchors' stand-up boxes have zero extent and the union term of the reference's IoU is
(y1 - x1 + 1) (oracle/targets.py), so with ground truths about 1 m across the IoU is roughly 1 / (y1 - x1 + area): negative
over most of the map, above the positive threshold only in a band near y = x - 2, and in the hundreds where the union
nearly cancels.  A slice of the grid therefore has to start inside that band to hold any positive at all."""
import functools

import numpy as np

from oracle import predict as op
from oracle import targets as ot

CLASS_NAMES = ("Car", "Pedestrian", "Cyclist")
BLOCK = 256                                              # threads of a workgroup in csrc/targets.hip and csrc/predict.hip
# (h, w) of a slice -> N = 2, 64, 130, 256, 270 anchors: less than a wave, one wave, a partial workgroup, one workgroup,
# one workgroup plus 14
SLICE_SHAPES = ((1, 1), (4, 8), (5, 13), (16, 8), (9, 15))
SLICE_ORIGIN = {"Car": (118, 25), "Pedestrian": (66, 22), "Cyclist": (66, 22)}          # (iy0, ix0): inside the positive band
TILES = 3
FULL_PAD, SLICE_PAD = 5.0, 1.0
# (seed, boxes per sample)
FULL_SEEDS = ((1, (3, 0, 40)), (3, (128, 7)))
SLICE_SEEDS = ((5, (5, 0, 12)), (4, (12,)))
EMPTY_SEED = (4, (0, 0))


def full_grid(cls_name):
    return ot.generate_anchors(cls_name)


def slice_grid(cls_name, hw, origin=None):
    iy0, ix0 = SLICE_ORIGIN[cls_name] if origin is None else origin
    return np.ascontiguousarray(ot.generate_anchors(cls_name)[iy0:iy0 + hw[0], ix0:ix0 + hw[1]])


def tiled_grid(cls_name, origin=None):
    """the (9,15) slice three times along the rows: (27,15,2,7), N = 810 — every anchor occurs in three different
    workgroups, so each box's best IoU is tied across workgroups and the FIRST occurrence has to win"""
    return np.concatenate([slice_grid(cls_name, SLICE_SHAPES[-1], origin)] * TILES, axis=0)


def grid_extent(cls_name, anchors=None):
    """(x0, x1, y0, y1): the class's range for the full grid, else the extent of the anchors' centres"""
    if anchors is None:
        c = ot.CLASSES[cls_name]
        return (*c["x"], *c["y"])
    a = anchors.reshape(-1, 7)
    return float(a[:, 0].min()), float(a[:, 0].max()), float(a[:, 1].min()), float(a[:, 1].max())


def gt_boxes(cls_name, seed, counts, extent, pad):
    """per sample, in this order: x, y ~ U(extent -+ pad), z ~ U(-2,-1), (h, w, l) = the anchor's size x U(0.9,1.1),
    r ~ U(-1.57,1.57); from 3 boxes on box 1 is a copy of box 0 (identical boxes tie; the first one must win)"""
    c = ot.CLASSES[cls_name]
    x0, x1, y0, y1 = extent
    rng = np.random.default_rng(seed)
    out = []
    for n in counts:
        b = np.stack([rng.uniform(x0 - pad, x1 + pad, n), rng.uniform(y0 - pad, y1 + pad, n), rng.uniform(-2, -1, n),
                      c["h"] * rng.uniform(0.9, 1.1, n), c["w"] * rng.uniform(0.9, 1.1, n), c["l"] * rng.uniform(0.9, 1.1, n),
                      rng.uniform(-1.57, 1.57, n)], axis=1).reshape(n, 7)
        if n >= 3:
            b[1] = b[0]
        out.append(b)
    return out


class TargetCase:
    """one class, one grid, one seed: anchors (h,w,2,7), the per-sample boxes, and the oracle's answer (computed once,
    read-only)"""

    def __init__(self, cls_name, grid, seed, counts, anchors, boxes):
        self.cls_name, self.grid, self.seed, self.counts = cls_name, grid, seed, tuple(counts)
        self.anchors, self.boxes = anchors, boxes
        self.shape = tuple(anchors.shape[:2])
        self.n_anchors = anchors.shape[0] * anchors.shape[1] * 2

    @property
    def id(self):
        return f"{self.cls_name}-{self.grid}-seed{self.seed}-B{len(self.counts)}"

    @functools.cached_property
    def ref(self):
        out = ot.generate_targets_from_boxes(self.boxes, self.shape, self.anchors, self.cls_name)
        for a in out:
            a.setflags(write=False)
        return out

    @functools.cached_property
    def iou(self):
        """per sample the oracle's (N, G) float32 IoU table"""
        a2d = ot.anchor_standup_2d(self.anchors)
        return [ot.bbox_iou(a2d, ot.gt_standup_2d(g)) for g in self.boxes]

    def stats(self):
        """what the case contains, summed over its samples, from the oracle's IoU tables alone"""
        c = ot.CLASSES[self.cls_name]
        s = dict(thr_pos=0, argmax_only=0, pos_and_neg=0, neg_iou=0, no_pos_box=0, cross_block_ties=0, inf_iou=0)
        for iou in self.iou:
            if iou.shape[1] == 0:
                continue
            with np.errstate(invalid="ignore"):
                thr = (iou > c["pos"]).any(axis=1)
                neg = (iou < c["neg"]).all(axis=1)
            best = iou.max(axis=0)
            idmax = np.argmax(iou, axis=0)
            am = np.zeros(iou.shape[0], dtype=bool)
            am[idmax[best > 0]] = True
            s["thr_pos"] += int(thr.sum())
            s["argmax_only"] += int((am & ~thr).sum())
            s["pos_and_neg"] += int(((am | thr) & neg).sum())
            s["neg_iou"] += int((iou < 0).sum())
            s["no_pos_box"] += int((best <= 0).sum())
            s["inf_iou"] += int(np.isinf(iou).sum())
            for k in np.flatnonzero(best > 0):
                s["cross_block_ties"] += int(len(set(np.flatnonzero(iou[:, k] == best[k]) // BLOCK)) > 1)
        return s


@functools.lru_cache(maxsize=None)
def target_case(cls_name, grid, seed, counts):
    """grid: 'full', 'tiled' or a slice's (h, w)"""
    if grid == "full":
        anchors, ext, pad = full_grid(cls_name), grid_extent(cls_name), FULL_PAD
    else:
        anchors = tiled_grid(cls_name) if grid == "tiled" else slice_grid(cls_name, grid)
        ext, pad = grid_extent(cls_name, anchors), SLICE_PAD
    name = grid if isinstance(grid, str) else f"{grid[0]}x{grid[1]}"
    return TargetCase(cls_name, name, seed, counts, anchors, gt_boxes(cls_name, seed, counts, ext, pad))


def full_cases():
    return [target_case(c, "full", s, n) for c in ("Pedestrian", "Cyclist") for s, n in FULL_SEEDS]


def slice_cases():
    return [target_case(c, hw, s, n) for c in CLASS_NAMES for hw in SLICE_SHAPES for s, n in SLICE_SEEDS]


def tiled_cases():
    return [target_case(c, "tiled", s, n) for c in CLASS_NAMES for s, n in SLICE_SEEDS]


def empty_cases():
    return [target_case(c, "full", *EMPTY_SEED) for c in ("Pedestrian", "Cyclist")] + \
           [target_case("Pedestrian", SLICE_SHAPES[-1], *EMPTY_SEED)]


def all_target_cases():
    return full_cases() + slice_cases() + tiled_cases() + empty_cases()


def last_occurrence_targets(case):
    """the oracle with the WRONG tie rule — each box's arg-max takes the LAST anchor of maximal IoU: what the tie test has
    to tell from the right answer (used by the host test only)"""
    real = np.argmax

    def argmax_last(a, axis=None):
        return a.shape[axis] - 1 - real(np.flip(a, axis=axis), axis=axis)
    np.argmax = argmax_last
    try:
        return ot.generate_targets_from_boxes(case.boxes, case.shape, case.anchors, case.cls_name)
    finally:
        np.argmax = real


def label_lines(cls_name, boxes, seed):
    """the boxes of one sample as KITTI label lines (targets.lidar_box_to_label_line) with lines of other classes mixed
    in at seeded places"""
    from voxelnet_amd.targets import lidar_box_to_label_line
    rng = np.random.default_rng(seed)
    others = [n for n in ("Car", "Van", "Cyclist", "Pedestrian", "Person_sitting", "DontCare") if n != cls_name]
    lines = [lidar_box_to_label_line(cls_name, b) for b in boxes]
    for k, name in enumerate(others):
        box = boxes[k % len(boxes)] if len(boxes) else np.array([10.0, 0.0, -1.5, 1.7, 0.6, 0.8, 0.1])
        lines.insert(int(rng.integers(0, len(lines) + 1)), lidar_box_to_label_line(name, box))
    return lines


# ------------------------------------------------------------------------------------------- candidate maps
PATCHES, PATCH = 3, 4          # per sample three patches of 4 x 4 cells x 2 rotations = 96 clustered candidates


@functools.lru_cache(maxsize=None)
def clustered_maps(shape, seed):
    """B = 2 maps on an (h, w) grid: probs below every threshold, except three patches per sample of (up to) 4 x 4 cells x
    2 rotations at 0.96 + 0.04 U — addressed by FLAT anchor index j = ((iy*w + ix)*2 + r) into probs[b].reshape(-1), since
    the reference reads the NCHW maps without a permute (oracle/predict.py).  Neighbouring anchors with small deltas: the
    NMS has something to suppress.  -> (probs (2,2,h,w), deltas (2,14,h,w)) float32, read-only"""
    h, w = shape
    rng = np.random.default_rng(seed)
    probs = (rng.random((2, 2, h, w)) * 0.9).astype(np.float32)
    deltas = (rng.standard_normal((2, 14, h, w)) * 0.3).astype(np.float32)
    ph, pw = min(PATCH, h), min(PATCH, w)
    for b in range(2):
        flat = probs[b].reshape(-1)
        for _ in range(PATCHES):
            iy0, ix0 = int(rng.integers(0, h - ph + 1)), int(rng.integers(0, w - pw + 1))
            for iy in range(iy0, iy0 + ph):
                for ix in range(ix0, ix0 + pw):
                    for r in range(2):
                        flat[(iy * w + ix) * 2 + r] = np.float32(0.96 + 0.04 * rng.random())
    probs.setflags(write=False)
    deltas.setflags(write=False)
    return probs, deltas


class DecodeCase:
    def __init__(self, cls_name, grid, seed):
        self.cls_name, self.grid, self.seed = cls_name, grid, seed
        self.anchors = full_grid(cls_name) if grid == "full" else slice_grid(cls_name, grid)
        self.shape = tuple(self.anchors.shape[:2])
        self.probs, self.deltas = clustered_maps(self.shape, seed)

    @property
    def id(self):
        return f"{self.cls_name}-{self.grid if isinstance(self.grid, str) else '%dx%d' % self.grid}-seed{self.seed}"

    @functools.cached_property
    def ref(self):
        """oracle.predict.predict_boxes: ([boxes (n,7)], [scores (n,)]) with the reference's constants"""
        rb, rs = op.predict_boxes(self.probs, self.deltas, self.anchors, self.cls_name)
        return [b.reshape(-1, 7) for b in rb], rs

    def candidates(self, score_thres=op.SCORE_THRES):
        return (self.probs.reshape(2, -1) >= np.float32(score_thres)).sum(axis=1)


DECODE_GRIDS = (("Pedestrian", "full"), ("Cyclist", "full"), ("Car", "full"), ("Pedestrian", (5, 13)), ("Cyclist", (5, 13)),
                ("Pedestrian", (9, 15)), ("Cyclist", (9, 15)))
DECODE_SEEDS = (13, 28)          # two seeds that hold NMS_MARGIN on every grid at every DECODE_PARAMS entry (5 and 6 do not)
# (score_thres, nms_thres, top_k): the reference's constants at the three pool sizes, and other thresholds
DECODE_PARAMS = ((op.SCORE_THRES, op.NMS_THRES, 20), (op.SCORE_THRES, op.NMS_THRES, 64), (op.SCORE_THRES, op.NMS_THRES, 1),
                 (0.97, 0.3, 20), (0.975, 0.05, 64), (0.97, 0.3, 1))
NMS_MARGIN = 1e-4          # no IoU the reference's walk evaluates may lie this close to the NMS threshold: the device's
#                            float32 boxes may differ by rtol 2.4e-7 / atol 1e-6, a few 1e-6 of IoU on a 0.6 m side


@functools.lru_cache(maxsize=None)
def decode_case(cls_name, grid, seed):
    return DecodeCase(cls_name, grid, seed)


def decode_cases():
    return [decode_case(c, g, s) for c, g in DECODE_GRIDS for s in DECODE_SEEDS]


def reference_walk(probs, deltas, anchors, cls_name, score_thres, nms_thres, top_k):
    """tests/detect_ref.py in stand-up mode with pre_top_k = post_top_k = top_k on ONE sample's maps (what vn_rpn_predict
    computes, with free constants) -> (boxes (k,7) f32, scores (k,) f32, number selected, smallest |IoU - nms_thres| over
    the IoUs the walk evaluated)"""
    import detect_ref as D
    idx = D.select(probs, score_thres, top_k)
    boxes = D.decode(deltas, anchors, idx, cls_name)
    keep, gap = D.nms(boxes, D.STANDUP, nms_thres, top_k)
    return boxes[keep], np.asarray(probs, dtype=np.float32).reshape(-1)[idx][keep], len(idx), gap


def tied_maps(case, top_k=20):
    """the case's maps with exact score ties: four neighbouring flat indices inside a cluster at one score above all
    others, and a group of seven equal scores that straddles the top_k cut (three inside, four outside) — of equal scores
    the LARGER flat index goes first (oracle/predict.py) -> (probs, deltas), probs a modified copy"""
    probs = case.probs.copy()
    for b in range(2):
        flat = probs[b].reshape(-1)
        cand = np.flatnonzero(flat >= np.float32(op.SCORE_THRES))
        order = cand[np.argsort(flat[cand], kind="stable")[::-1]]
        j0 = int(order[0]) // 4 * 4
        flat[j0:j0 + 4] = np.float32(0.9995)                      # 2 cells x 2 rotations: neighbours of one cluster
        cand = np.flatnonzero(flat >= np.float32(op.SCORE_THRES))
        order = cand[np.argsort(flat[cand], kind="stable")[::-1]]
        v = flat[order[top_k - 3]]                                 # ranks top_k-2 .. top_k+4 (1-based) share v
        flat[order[top_k - 3:top_k + 4]] = v
    probs.setflags(write=False)
    return probs, case.deltas
