"""NumPy restatement of the augmentation specification (voxelnet_amd/augment.py + csrc/augment.hip; the reference's
pcl_augmentation, voxelnet/dataset.py:122-219) — the arbiter of the device kernel and of the host draw.

Written on its own from the specification, sharing with the package only the two primitives the specification names
(targets.label_to_gt_box_3d for the starting boxes, targets.gt_standup_boxes for the footprint hull):
  - every float64 expression is elementwise and spelled exactly as the specification writes it (no matmul: a BLAS may
    fuse a multiply and an add), rounded once to float32;
  - the box loop is the sequential in-place one: box 0 moves its points, then box 1 tests the moved cloud, ...;
  - the collision test works on corners (projection of both footprints' corners on each edge direction), not on the
    centre-distance form the package uses.
"""
import numpy as np

from voxelnet_amd.targets import _limit_angle, gt_standup_boxes, label_to_gt_box_3d


def move_points(xyz32, tx, ty, tz, c, s):
    """rigid motion of (M,3) float32 rows -> (M,3) float32: promote, translate, rotate the row vector, round once"""
    X = xyz32[:, 0].astype(np.float64) + tx
    Y = xyz32[:, 1].astype(np.float64) + ty
    Z = xyz32[:, 2].astype(np.float64) + tz
    out = np.empty_like(xyz32)
    out[:, 0] = (X * c + Y * s).astype(np.float32)
    out[:, 1] = (-(X * s) + Y * c).astype(np.float32)
    out[:, 2] = Z.astype(np.float32)
    return out


def move_box(box, tx, ty, tz, rz):
    c, s = np.cos(rz), np.sin(rz)
    X, Y, Z = box[0] + tx, box[1] + ty, box[2] + tz
    return np.array([X * c + Y * s, -(X * s) + Y * c, Z, box[3], box[4], box[5], _limit_angle(box[6] - rz)])


def _corners(box):
    x, y, w, l, r = box[0], box[1], box[4], box[5], box[6]
    c, s = np.cos(r), np.sin(r)
    return [(x + fx * c - fy * s, y + fx * s + fy * c) for fx, fy in ((-l / 2, w / 2), (-l / 2, -w / 2), (l / 2, -w / 2), (l / 2, w / 2))]


def overlap(a, b):
    """positive-area overlap of two rotated footprints: no edge direction of either separates the corner sets"""
    ca, cb = _corners(a), _corners(b)
    for poly in (ca, cb):
        for i in range(2):                                    # a rectangle has two distinct edge directions
            ex, ey = poly[i + 1][0] - poly[i][0], poly[i + 1][1] - poly[i][1]
            norm = np.hypot(ex, ey)
            if norm == 0.0:
                return False                                  # a degenerate footprint has no area to share
            pa = [(px * ex + py * ey) / norm for px, py in ca]
            pb = [(px * ex + py * ey) / norm for px, py in cb]
            if min(pa) >= max(pb) or min(pb) >= max(pa):
                return False
    return True


def bounds(box):
    x0, y0, x1, y1 = gt_standup_boxes(np.asarray(box, dtype=np.float64).reshape(1, 7))[0]
    return (np.array([x0, y0, np.float32(box[2])], np.float32), np.array([x1, y1, np.float32(box[2] + box[3])], np.float32))


def draw(labels):
    """the host draw from the global np.random state -> dict(mode, choice, before, after, table / angle / factor);
    table = [(lo (3,) f32, hi (3,) f32, tx, ty, tz, cos rz, sin rz)] of the accepted perturbations in label order"""
    choice = np.random.randint(0, 10)
    boxes = label_to_gt_box_3d([labels], "", "lidar")[0].copy()
    out = dict(choice=int(choice), before=boxes.copy())
    if choice >= 7:
        table = []
        for idx in range(len(boxes)):
            for _attempt in range(100):
                rz = np.random.uniform(-np.pi / 10, np.pi / 10)
                tx = np.random.normal()
                ty = np.random.normal()
                tz = np.random.normal()
                cand = move_box(boxes[idx], tx, ty, tz, rz)
                if any(overlap(cand, boxes[idy]) for idy in range(idx)):
                    continue
                lo, hi = bounds(boxes[idx])
                table.append((lo, hi, tx, ty, tz, np.cos(rz), np.sin(rz)))
                boxes[idx] = cand
                break
        out.update(mode="boxes", table=table)
    elif choice >= 4:
        angle = np.random.uniform(-np.pi / 4, np.pi / 4)
        for idx in range(len(boxes)):
            boxes[idx] = move_box(boxes[idx], 0.0, 0.0, 0.0, angle)
        out.update(mode="rotate", angle=float(angle))
    else:
        factor = np.random.uniform(0.95, 1.05)
        boxes[:, 0:6] *= factor
        out.update(mode="scale", factor=float(factor))
    out["after"] = boxes
    return out


def apply(cloud, d):
    """cloud (N,4) float32 -> the augmented copy; d: a draw() dict (or the same keys made from the package's params)"""
    pts = np.array(cloud, dtype=np.float32, copy=True)
    if d["mode"] == "boxes":
        for lo, hi, tx, ty, tz, c, s in d["table"]:           # sequential and in place, like the reference's loop
            with np.errstate(invalid="ignore"):
                inside = np.ones(len(pts), dtype=bool)
                for a in range(3):
                    inside &= (pts[:, a] >= np.float32(lo[a])) & (pts[:, a] <= np.float32(hi[a]))
            pts[inside, :3] = move_points(pts[inside, :3], tx, ty, tz, c, s)
    elif d["mode"] == "rotate":
        pts[:, :3] = move_points(pts[:, :3], 0.0, 0.0, 0.0, np.cos(d["angle"]), np.sin(d["angle"]))
    elif d["mode"] == "scale":
        f = np.float32(d["factor"])
        pts[:, 0] = pts[:, 0] * f
        pts[:, 1] = pts[:, 1] * f
        pts[:, 2] = pts[:, 2] * f
    else:
        raise ValueError(d["mode"])
    return pts


def from_params(p):
    """the package's AugmentParams -> the dict form apply() takes"""
    return dict(mode=p.mode, angle=p.angle, factor=p.factor,
                table=[(r["lo"], r["hi"], r["t"][0], r["t"][1], r["t"][2], r["c"], r["s"]) for r in p.table])
