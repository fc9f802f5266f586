"""Inputs of the SimOTA target assignment, shared by tests/test_ota_host.py — which asserts ON THE
REFERENCE ALONE (tests/ota_ref.py) that no decision of any (case, metric, q) lies within MARGIN — and tests/test_gpu_ota.py.
Anchor grids and boxes are tests/assign_cases.py's and tests/atss_cases.py's; the prediction maps come from a seeded generator:
deltas = the encoded targets of a perturbed copy of the anchor's nearest box plus noise, so that v spreads over (0, 1), probs
uniform in (0.01, 0.99).  Special maps and radii are cases of their own (see cases())."""
import functools

import numpy as np

import assign_cases as C
import atss_cases as AC
import label_cases as L
import ota_ref as T

MARGIN = 1e-6          # the issue's: every decision of the reference stands off by more than this
METRICS = T.METRICS
QS = (1, 10, 16)          # the smallest, YOLOX's default, VN_OTA_MAX_Q
IOU_WEIGHT = 3.0
OVERFLOW_D3 = 800.0          # exp overflows float64 above 709.78
PITCHES = 2.5          # the default radius in site pitches (targets.OTA_RADIUS_PITCHES)


def pitch(anchors):
    """targets.site_pitch restated: the larger of the mean column and row pitch"""
    h, w = anchors.shape[:2]
    p = ([abs(anchors[0, -1, 0, 0] - anchors[0, 0, 0, 0]) / (w - 1)] if w > 1 else []) + \
        ([abs(anchors[-1, 0, 0, 1] - anchors[0, 0, 0, 1]) / (h - 1)] if h > 1 else [])
    return float(max(p))


def encode_all(a, g, anchor_h):
    """assign_ref.encode's expressions on arrays: anchors a (N,7), one box per anchor g (N,7) -> (N,7) float64"""
    diag = np.sqrt(a[:, 4] ** 2 + a[:, 5] ** 2)
    return np.stack([(g[:, 0] - a[:, 0]) / diag, (g[:, 1] - a[:, 1]) / diag, (g[:, 2] - a[:, 2]) / anchor_h, np.log(g[:, 3] / a[:, 3]),
                     np.log(g[:, 4] / a[:, 4]), np.log(g[:, 5] / a[:, 5]), g[:, 6] - a[:, 6]], axis=1)


def site_layout(per_anchor, shape):
    """(N, c) values per anchor n = 2 * site + a -> (c * 2, h, w) float32: channel a * c + j of site s holds [2s + a, j]"""
    h, w = shape
    c = per_anchor.shape[1]
    return np.ascontiguousarray(per_anchor.reshape(h * w, 2, c).transpose(1, 2, 0).reshape(2 * c, h, w).astype(np.float32))


def seeded_maps(anchors, boxes, anchor_h, seed):
    """-> probs (B,2,h,w), deltas (B,14,h,w) float32.  Per anchor: its nearest valid box (centre distance), moved by up to
    0.6 m, resized by up to 15 %, turned by up to 0.2 rad — each scaled by a per-anchor factor in (0, 1) —, encoded on the anchor,
    plus N(0, 0.01) noise; a sample without a valid box gets N(0, 0.1) deltas."""
    rng = np.random.default_rng(seed)
    a = anchors.reshape(-1, 7)
    N, shape = a.shape[0], anchors.shape[:2]
    probs, deltas = [], []
    for g in boxes:
        ok = np.array([T.box_valid(q) for q in g], dtype=bool)
        if ok.any():
            gv = g[ok]
            near = gv[np.argmin((a[:, None, 0] - gv[None, :, 0]) ** 2 + (a[:, None, 1] - gv[None, :, 1]) ** 2, axis=1)].copy()
            f = rng.uniform(0.0, 1.0, (N, 1))
            near[:, :3] += f * rng.uniform(-1, 1, (N, 3)) * (0.6, 0.6, 0.2)
            near[:, 3:6] *= 1.0 + f * rng.uniform(-0.15, 0.15, (N, 3))
            near[:, 6] += f[:, 0] * rng.uniform(-0.2, 0.2, N)
            d = encode_all(a, near, anchor_h) + rng.normal(0.0, 0.01, (N, 7))
        else:
            d = rng.normal(0.0, 0.1, (N, 7))
        deltas.append(site_layout(d, shape))
        probs.append(site_layout(rng.uniform(0.01, 0.99, (N, 1)), shape))
    return np.stack(probs), np.stack(deltas)


class OtaCase:
    """anchors (h,w,2,7), per-sample boxes, the prediction maps and the call's parameters, with the reference's answers computed
    once and read-only"""

    def __init__(self, name, base, probs, deltas, radius=None, qs=QS):
        self.id, self.cls_name, self.anchors, self.boxes = name, base.cls_name, base.anchors, base.boxes
        self.shape, self.n_anchors, self.anchor_h = base.shape, base.n_anchors, base.anchor_h
        self.probs, self.deltas, self.qs, self.iou_weight = probs, deltas, tuple(qs), IOU_WEIGHT
        self.radius = PITCHES * pitch(base.anchors) if radius is None else float(radius)
        for m in (probs, deltas):
            m.setflags(write=False)
        B = len(self.boxes)
        assert probs.shape == (B, 2, *self.shape) and deltas.shape == (B, 14, *self.shape)

    @functools.lru_cache(maxsize=None)
    def pairs(self):
        return [T.pair_values(self.anchors, b, p, d, self.radius) for b, p, d in zip(self.boxes, self.probs, self.deltas)]

    @functools.lru_cache(maxsize=None)
    def ref(self, metric, q):
        out = [T.assign_sample(self.anchors, b, pr, metric, q, self.iou_weight, self.anchor_h) for b, pr in zip(self.boxes, self.pairs())]
        for s in out:
            for v in s.values():
                for x in (v if isinstance(v, list) else [v]):
                    x.setflags(write=False)
        return out

    @functools.lru_cache(maxsize=None)
    def guard(self, metric, q):
        """asserts the guard on the reference alone -> the smallest gap of each sort over the samples"""
        gaps = [T.guard(self.anchors, b, p, d, s, self.radius, MARGIN)
                for b, p, d, s in zip(self.boxes, self.probs, self.deltas, self.ref(metric, q))]
        return {key: min(g[key] for g in gaps) for key in gaps[0]}


def _seeded(name, base, seed, **kw):
    return OtaCase(name, base, *seeded_maps(base.anchors, base.boxes, base.anchor_h, seed), **kw)


def _atss(name):
    return next(c for c in AC.cases() if c.id == name).base


def _candidate(case_pairs, b, k, both=True, skip=0):
    """-> (site, a) of a candidate of box k of sample b (in_box and in_ctr when `both`), the skip-th such"""
    pk = case_pairs[b][k]
    n = int(pk["n"][np.flatnonzero(pk["both"] == both)[skip]])
    return divmod(n, 2)


def zero_maps():
    """all-zero deltas (every prediction is its anchor) with one constant p, on the tiled grid: the three copies of an anchor
    have bit-equal inputs, equal costs, and the smallest n of a tie ranks first"""
    base = _atss("Car-tiled")
    B = len(base.boxes)
    return OtaCase("Car-tiled-zero-deltas", base, np.full((B, 2, *base.shape), 0.37, dtype=np.float32),
                   np.zeros((B, 14, *base.shape), dtype=np.float32))


def odd_values():
    """the hand-made frames with three entries of sample 0 overwritten, each at an anchor inside box 0's footprint and radius:
    p = 0 (counts as 1e-12), p = NaN (likewise), and d3 = OVERFLOW_D3 (the float64 exp overflows: the decoded height is inf,
    v = 0; at 200 it does not yet — exp(200) = 7e86 is finite, and the 3D IoU would be 1e-87, not 0)"""
    base = C.hand_frames()
    probs, deltas = seeded_maps(base.anchors, base.boxes, base.anchor_h, 31)
    plain = OtaCase("tmp", base, probs.copy(), deltas.copy())
    w = base.shape[1]
    for i, what in enumerate(("p0", "pnan", "d3")):
        s, a = _candidate(plain.pairs(), 0, 0, skip=2 * i)
        if what == "d3":
            deltas[0, 7 * a + 3, s // w, s % w] = OVERFLOW_D3
        else:
            probs[0, a, s // w, s % w] = 0.0 if what == "p0" else np.nan
    return OtaCase("Car-hand-odd-values", base, probs, deltas)


def scaled_box(q_special=7):
    """one box on the hand-made frames' grid; every candidate predicts that box with its length scaled by 0.8 (x 1 +- 0.004), so
    every v is 0.8 +- 0.004 in both metrics, and the p of the candidates fall by a factor 0.93 from one to the next in a
    shuffled order: at q = 7 sum_k is about 5.6, dyn_k = 5, and the five largest p inside footprint and radius win"""
    h = C.hand_frames()
    a = h.anchors.reshape(-1, 7)
    x0, x1, y0, y1 = a[:, 0].min(), a[:, 0].max(), a[:, 1].min(), a[:, 1].max()
    box = np.array([[x0 + 0.47 * (x1 - x0), y0 + 0.53 * (y1 - y0), -1.7, 1.5, 1.65, 4.0, 0.3]])
    base = C.AssignCase("Car-hand-one-box", "Car", h.anchors, [box])
    rng = np.random.default_rng(17)
    N = a.shape[0]
    pred = np.repeat(box, N, axis=0)
    pred[:, 5] *= 0.8 * (1.0 + rng.uniform(-0.004, 0.004, N))
    d = encode_all(a, pred, base.anchor_h)
    radius = PITCHES * pitch(h.anchors)
    eu, ew, ex, ey = T.offsets(a, box[0], radius)
    cand = np.flatnonzero(((eu <= 0) & (ew <= 0)) | ((ex <= 0) & (ey <= 0)))
    p = np.full((N, 1), 1e-3)
    p[rng.permutation(cand), 0] = 0.95 * 0.93 ** np.arange(cand.size)
    return OtaCase("Car-hand-scaled-box", base, site_layout(p, base.shape)[None], site_layout(d, base.shape)[None],
                   qs=QS + (q_special,))


def wide_radius():
    """a radius larger than the grid: every anchor is a candidate of both boxes of sample 0.  Sample 1 holds 128 invalid boxes
    (w = 0) and samples 2..7 none, so that B * max_gt = 1024 and the scan takes the 768 sites in ONE chunk: 12 sites, 24
    candidates per lane — more than q, the bounded lists overflow."""
    h = C.hand_frames()
    a = h.anchors.reshape(-1, 7)
    x0, x1, y0, y1 = a[:, 0].min(), a[:, 0].max(), a[:, 1].min(), a[:, 1].max()

    def car(fx, fy, r, w=1.65):
        return [x0 + fx * (x1 - x0), y0 + fy * (y1 - y0), -1.7, 1.5, w, 4.0, r]
    frames = [[car(0.21, 0.23, 0.2), car(0.79, 0.77, -0.4)], [car(0.5, 0.5, 0.1, w=0.0)] * 128] + [[]] * 6
    base = C.AssignCase("Car-hand-wide", "Car", h.anchors, [np.array(f, dtype=np.float64).reshape(-1, 7) for f in frames])
    return _seeded("Car-hand-wide-radius", base, 41, radius=100.0)


def full_grid():
    """the full Car grid (70,400 anchors), B = 2 with 8 and 128 boxes"""
    anchors = L.full_grid("Car")
    boxes = L.gt_boxes("Car", 5, (8, 128), L.grid_extent("Car"), 0.0)
    return _seeded("Car-full-8-128", C.AssignCase("Car-full-8-128", "Car", anchors, boxes), 54)


@functools.lru_cache(maxsize=None)
def cases():
    seeded = [("Car-1x1", 1, dict(radius=1.0)), ("Car-5x13", 2, {}), ("Car-9x15", 3, {}), ("Car-5x13-128boxes", 4, {}),
              ("Car-hand", 5, {}), ("Car-atss-extra", 6, {}), ("Pedestrian-9x15", 8, {})]
    out = [_seeded(name, _atss(name), seed, **kw) for name, seed, kw in seeded]
    out.append(_seeded("Car-hand-radius0", C.hand_frames(), 8, radius=0.0))
    out += [zero_maps(), odd_values(), scaled_box(), wide_radius(), full_grid()]
    return tuple(out)


def combos():
    """every (case, metric, q) the GPU test runs"""
    return [(c, metric, q) for c in cases() for metric in METRICS for q in c.qs]


def combo_id(combo):
    return "%s-%s-q%d" % (combo[0].id, combo[1], combo[2])
