"""Inputs of the direction-classifier head's tests, shared by tests/test_dir_host.py — which asserts
the guards ON THE REFERENCE ALONE (tests/dir_ref.py) — and tests/test_gpu_dir_head.py."""
import functools

import numpy as np

import dir_ref as R
from oracle import targets as ot

C = 768
HEAD_SHAPES = ((1, 5), (2, 70), (3, 257))          # fewer rows than one wave; a sample boundary inside a tile + a partial tail;
#                                                    an odd row count over several workgroups
STRIDES = (768, 1024)
SENTINEL = 777.25                                  # exact in bf16 and fp32
PATTERNS = ("zero", "first_last", "spread", "g0_zero", "all")
LOSS_SHAPES = ((3, 7, 5), (2, 16, 24), (2, 17, 15))          # tests/test_gpu_focal_loss.py's maps; no positive in (3,7,5)'s last sample
OFFSETS = (np.pi / 4, 0.0)
# headings clear of the bin edges under both offsets (0.8 is 0.015 from an edge under pi/4), their turns by pi, and some
# beyond +-2 pi; all four quadrants
YAWS = (0.2, -1.3, 2.0, 0.2 - np.pi, -1.3 + np.pi, 2.0 - np.pi, 0.2 + 2 * np.pi, -1.3 - 2 * np.pi, 2.0 + 4 * np.pi, -2.9, 2.6 - 4 * np.pi)
HAND_LOGITS = (30.0, -30.0, 1e-3, -1e-3, 0.0)          # at the first five positives


@functools.lru_cache(maxsize=None)
def head_case(B, S, seed=11):
    """-> dict of float32 arrays: x (B*S, 768), w (2, 768), bias (2,), d_cat (B*S, 768) — read-only"""
    rng = np.random.default_rng(seed + 100 * B + S)
    M = B * S
    out = {"x": rng.standard_normal((M, C)).astype(np.float32),
           "w": (rng.standard_normal((2, C)) * 0.05).astype(np.float32),
           "bias": rng.standard_normal(2).astype(np.float32),
           "d_cat": rng.standard_normal((M, C)).astype(np.float32)}
    for v in out.values():
        v.setflags(write=False)
    return out


def grad_pattern(name, B, S, seed=17):
    """-> g (B*S, 2) float32: the head's upstream gradient by row, and the sorted list of rows that are not all zero"""
    M = B * S
    rng = np.random.default_rng(seed + M)
    g = np.zeros((M, 2), dtype=np.float32)
    full = (rng.standard_normal((M, 2)) * 0.1).astype(np.float32)
    full[full == 0] = 0.1
    if name == "zero":
        rows = []
    elif name == "first_last":
        rows = sorted({0, M - 1})
    elif name == "spread":          # rows of different 256-row workgroups of the compaction where there are several
        rows = sorted({1 % M, M // 3, M // 2 + 1, (5 * M) // 6})
    elif name == "g0_zero":
        rows = sorted({M // 2, M - 1})
    elif name == "all":
        rows = list(range(M))
    else:
        raise ValueError(name)
    g[rows] = full[rows]
    if name == "g0_zero":
        g[M // 2, 0] = 0.0
        g[M - 1, 1] = -0.0
    if name == "spread":
        g[M // 2, :] = -0.0          # a row of two negative zeros is not listed
        g[M // 2 + 1, 1] = 0.0
    listed = [m for m in range(M) if g[m, 0] != 0 or g[m, 1] != 0]
    return g, listed


@functools.lru_cache(maxsize=None)
def loss_case(shape, seed=23):
    """-> dict: logits (B,2,h*w) f32, pos (B,h,w,2) f32, targets (B,h,w,14) f32, anchors (h,w,2,7) f64, n_exact_zero"""
    B, h, w = shape
    rng = np.random.default_rng(seed + h * w)
    anchors = np.ascontiguousarray(ot.generate_anchors("Car")[:h, :w])
    pos = (rng.random((B, h, w, 2)) < 0.12).astype(np.float32)
    if shape == LOSS_SHAPES[0]:
        pos[-1] = 0.0
    pos[0, 0, 0, :] = 1.0                                     # both rotations are among the positives
    assert int(pos.sum()) >= len(HAND_LOGITS)
    return _loss_inputs(pos, anchors, rng)


def _loss_inputs(pos, anchors, rng, hand=HAND_LOGITS):
    """targets and logits for the given positives: YAWS in turn as the matched headings, the `hand` logits at the first
    positives in the logits' layout"""
    B, h, w, _ = pos.shape
    targets = (rng.standard_normal((B, h, w, 14)) * 0.3).astype(np.float32)
    k = 0
    for idx in np.argwhere(pos != 0):
        b, y, x, a = (int(v) for v in idx)
        targets[b, y, x, 7 * a + 6] = np.float32(YAWS[k % len(YAWS)] - anchors[y, x, a, 6])
        k += 1
    logits = (rng.standard_normal((B, 2, h * w)) * 2.0).astype(np.float32)
    logits[np.abs(logits) < 1e-2] = 0.5
    p = np.argwhere(R.site_layout(pos) != 0)
    for (b, a, s), z in zip(p, hand):
        logits[b, a, s] = z
    out = {"logits": logits, "pos": pos, "targets": targets, "anchors": anchors}
    for v in out.values():
        v.setflags(write=False)
    out["n_exact_zero"] = sum(z == 0.0 for z in hand[:len(p)])
    return out


# The two loops of the loss' scaffold (csrc/rpn_common.h) that no LOSS_SHAPES entry reaches: tests/iou_loss_ref.py's
# SEAM_CASES, shapes and planted flat elements of pos (2 * global site + rotation) alike; the reasons are stated there.
SEAM_CASES = {
    (1, 33, 63): (0, 4095, 4096, 4157),
    (2, 129, 255): (0, 2 * 255, 2 * 256 + 1, 2 * 32894 + 1, 2 * 32895, 2 * 40000, 2 * 65535, 2 * 65536 + 1, 2 * 65789 + 1),
}


@functools.lru_cache(maxsize=None)
def seam_case(shape, seed=37):
    """loss_case's dict for a SEAM_CASES shape: the positives exactly the planted elements; the Car anchors' two rotations
    at every site (the loss reads the yaw column only; (2,129,255) is wider than the Car grid)"""
    B, h, w = shape
    rng = np.random.default_rng(seed + h * w)
    anchors = np.ascontiguousarray(np.broadcast_to(ot.generate_anchors("Car")[:1, :1], (h, w, 2, 7)))
    pos = np.zeros(B * h * w * 2, dtype=np.float32)
    pos[list(SEAM_CASES[shape])] = 1.0
    # HAND_LOGITS from its second entry: the four positives of (1,33,63) then hold the exact 0, and both offsets see hits and misses
    return _loss_inputs(pos.reshape(B, h, w, 2), anchors, rng, HAND_LOGITS[1:])


def rectify_case(seed=29):
    """B = 4 (the issue's two samples, one with count 0, one with a count above K), K = 37, 64 sites"""
    rng = np.random.default_rng(seed)
    B, K, S = 4, 37, 64
    boxes = rng.standard_normal((B, K, 7)).astype(np.float32)
    yaw = np.array([YAWS[i % len(YAWS)] + 0.01 * (i // len(YAWS)) for i in range(B * K)]).reshape(B, K)
    boxes[..., 6] = yaw.astype(np.float32)
    idx = rng.integers(0, 2 * S, size=(B, K)).astype(np.int32)
    counts = np.array([37, 5, 0, 50], dtype=np.int32)
    logits = (rng.standard_normal((B, 2, S)) * 2.0).astype(np.float32)
    logits[np.abs(logits) < 1e-2] = 0.5
    logits[0, idx[0, 0] & 1, idx[0, 0] >> 1] = 0.0          # the one exact 0: bin 0
    return {"boxes": boxes, "idx": idx, "counts": counts, "logits": logits, "S": S}


# ---- the round trip: frames of well-separated cars whose headings cover both bins, as KITTI label lines
ROUND_TRIP_FRACTIONS = (((0.2, 0.25), (0.75, 0.3), (0.3, 0.75), (0.8, 0.8)), ((0.3, 0.4), (0.7, 0.65)), ())
ROUND_TRIP_YAWS = (0.2, 0.2 - np.pi, -1.3, -1.3 + np.pi, 2.0, 2.0 - np.pi)
ROUND_TRIP_SIZES = ((1.5, 1.6, 3.9), (1.6, 1.7, 4.2), (1.45, 1.55, 3.6))          # assign_cases.round_trip_frames' (h, w, l)


def round_trip_anchors():
    return np.ascontiguousarray(ot.generate_anchors("Car")[100:124, 60:92])


def round_trip_frames(anchors):
    """-> (label lines per frame, lidar boxes per frame as kitti_ref reads those lines back: the heading kept).
    The lines are tests/kitti_ref.label_line's — the 2D box and alpha of the projected box, six decimals — because the
    image-plane evaluator matches by the label's 2D box and scores the heading by its alpha; tests/eval_ref.label_line
    writes a fixed 2D box and alpha 0, under which no detection can match in the image."""
    import kitti_ref as K
    a = np.asarray(anchors).reshape(-1, 7)
    x0, x1, y0, y1 = a[:, 0].min(), a[:, 0].max(), a[:, 1].min(), a[:, 1].max()
    frames, boxes, i = [], [], 0
    for fr in ROUND_TRIP_FRACTIONS:
        lines = []
        for fx, fy in fr:
            h, w, l = ROUND_TRIP_SIZES[i % 3]
            lines.append(K.label_line("Car", [x0 + fx * (x1 - x0), y0 + fy * (y1 - y0), -1.7, h, w, l, ROUND_TRIP_YAWS[i]], digits=6))
            i += 1
        frames.append(lines)
        boxes.append(K.frame_ground_truth(lines, "Car")["boxes"])
    return frames, boxes
