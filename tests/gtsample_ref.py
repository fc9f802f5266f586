"""NumPy / plain-Python restatement of the ground-truth database sampling specification (voxelnet_amd/gtsample.py +
csrc/gtsample.hip) — the arbiter of the device kernels, of the database and of the host draw.

Written on its own from the specification; it shares with the package only the primitive the specification names
(targets.label_to_gt_box_3d for a label line's box) and takes its collision test from tests/augment_ref.py (corner
projections), not the package's centre-distance form:
  - inside() works from the (7,) lidar box itself, every float64 expression elementwise and spelled as the
    specification writes it (no matmul: a BLAS may fuse a multiply and an add);
  - index / counts / paste are the plain definitions over the per-box masks;
  - the draw is the sequential loop of the specification on the global np.random state.
"""
import numpy as np

from augment_ref import overlap
from voxelnet_amd.targets import label_to_gt_box_3d

MAX_BOXES = 128


def entry(box):
    """(7,) lidar box (x, y, z, h, w, l, r) -> the eight float64 fields x, y, z0, z1, hl, hw, c, s"""
    x, y, z, h, w, l, r = (np.float64(v) for v in box)
    return x, y, z, z + h, l / 2, w / 2, np.cos(r), np.sin(r)


def inside_entry(cloud, e):
    """(N,) bool for explicit table fields (tests of hl < 0 or NaN fields)"""
    x, y, z0, z1, hl, hw, c, s = (np.float64(v) for v in e)
    px = cloud[:, 0].astype(np.float64)
    py = cloud[:, 1].astype(np.float64)
    pz = cloud[:, 2].astype(np.float64)
    with np.errstate(invalid="ignore"):
        dx = px - x
        dy = py - y
        u = dx * c + dy * s
        v = -(dx * s) + dy * c
        return (np.abs(u) <= hl) & (np.abs(v) <= hw) & (pz >= z0) & (pz <= z1)


def inside(cloud, box):
    return inside_entry(np.asarray(cloud, dtype=np.float32).reshape(-1, 4), entry(box))


def masks(cloud, boxes):
    cloud = np.asarray(cloud, dtype=np.float32).reshape(-1, 4)
    return np.array([inside(cloud, b) for b in boxes], dtype=bool).reshape(len(boxes), cloud.shape[0])


def index_counts(cloud, boxes):
    """-> (index (N,) int32: lowest box holding the point, else -1; counts (G,) int32)"""
    m = masks(cloud, boxes)
    index = np.full(m.shape[1], -1, dtype=np.int32)
    for j in range(m.shape[0] - 1, -1, -1):
        index[m[j]] = j
    return index, m.sum(1).astype(np.int32)


def paste(cloud, boxes, obj, cap=None):
    """-> (out (cap,4) float32 — kept scene rows in order, obj, NaN rows —, count)"""
    cloud = np.asarray(cloud, dtype=np.float32).reshape(-1, 4)
    obj = np.asarray(obj, dtype=np.float32).reshape(-1, 4)
    keep = ~np.isnan(cloud[:, :3]).any(1)
    if len(boxes):
        keep &= ~masks(cloud, boxes).any(0)
    cap = len(cloud) + len(obj) if cap is None else cap
    out = np.full((cap, 4), np.nan, dtype=np.float32)
    k = int(keep.sum())
    out[:k] = cloud[keep]
    out[k:k + len(obj)] = obj
    return out, k + len(obj)


def line_box(line):
    return label_to_gt_box_3d([[line]], "", "lidar")[0][0]


def database(frames, classes=("Car",)):
    """frames: [(tag, cloud, lines)] -> [dict(cls, tag, box, points, line)]"""
    out = []
    for tag, cloud, lines in frames:
        for line in lines:
            if line.split()[0] not in classes:
                continue
            box = line_box(line)
            out.append(dict(cls=line.split()[0], tag=str(tag), box=box, points=cloud[inside(cloud, box)], line=line))
    return out


def draw(db, labels, tag, per_class, min_points=5):
    """the host draw from the global np.random state -> dict(boxes (G,7), points (M,4), lines)"""
    existing = [line_box(line) for line in labels]
    taken = []
    for cls, target in per_class.items():
        want = max(0, target - len([1 for line in labels if line.split()[0] == cls]))
        pool = [e for e in db if e["cls"] == cls and len(e["points"]) >= min_points and e["tag"] != str(tag)]
        if want == 0 or len(pool) == 0:
            continue
        order = np.random.permutation(len(pool))[:want]
        for j in order:
            cand = pool[j]
            if len(taken) == MAX_BOXES:
                break
            if any(overlap(cand["box"], b) for b in existing):
                continue
            if any(overlap(cand["box"], t["box"]) for t in taken):
                continue
            taken.append(cand)
    boxes = np.array([t["box"] for t in taken], dtype=np.float64).reshape(-1, 7)
    points = np.concatenate([t["points"] for t in taken] + [np.zeros((0, 4), np.float32)]).astype(np.float32)
    return dict(boxes=boxes, points=points, lines=[t["line"] for t in taken])
