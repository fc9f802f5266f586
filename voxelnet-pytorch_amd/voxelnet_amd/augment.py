"""Point-cloud augmentation of the input pipeline — the reference's `pcl_augmentation` (voxelnet/dataset.py:122-219,
paper section 3.2: per-box perturbation, global rotation, global scaling) split where the work splits:

  host   (this module, O(boxes) NumPy): the random draw, the collision test between perturbed boxes (`calc_iou2d`,
         dataset.py:222-240), the moved boxes (`box_transform`, :254; `corner_to_center_box3d`, :305-384) and their
         label lines
  device (csrc/augment.hip, `vn_augment_points`): the per-point moves (`point_transform`, :264), on the pipeline's stream
         between the field-of-view crop and the voxelizer — there is no CPU path for the points.

`DeviceCollate(..., augment=True)` / `DeviceBatcher(..., augment=True)` (dataset.py) run the three functions below per
sample.  Stated divergences from the reference: the collision test is the exact geometric one (separating
axes, float64) instead of a cv2 rasterisation; a moved box is the closed form (centre moved like a point, r' = r - rz)
instead of the edge averages of its float32 corners.

The rigid motion (point_transform): translate, then multiply the ROW vector by the z-rotation matrix — a rotation by
-rz about the LIDAR ORIGIN, not about the box centre:
    X = x + tx, Y = y + ty, Z = z + tz;   x' = X*c + Y*s,   y' = -(X*s) + Y*c,   z' = Z      (c = cos rz, s = sin rz)

A second augmentation of the same stage is the COMPOSED recipe of SECOND / PointPillars / OpenPCDet (`ComposeRecipe`,
`draw_compose`, `compose_labels`, `compose_points_device`): per-object noise — every object with
its own points, turned about ITS OWN centre, placed where it collides with nothing — then a flip, a global rotation, a
scaling and optionally a global translation, all five for every sample, in one launch (`vn_augment_compose`).
`DeviceCollate(..., augment=ComposeRecipe())` runs it; `augment=True` stays the reference's one-of-three draw above."""
import ctypes
from dataclasses import dataclass, field
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib
from .targets import _limit_angle, gt_standup_boxes, label_to_gt_box_3d, lidar_box_to_label_line

MAX_BOXES = _lib.VN_AUGMENT_MAX_BOXES
MAX_ATTEMPTS = 100          # dataset.py:122-219: tries per box before it is left alone
# one entry of the device box table: vnAugmentBox (include/voxelnet_hip.h), 64 bytes
BOX_DTYPE = np.dtype([("lo", "<f4", 3), ("hi", "<f4", 3), ("t", "<f8", 3), ("c", "<f8"), ("s", "<f8")], align=True)
assert BOX_DTYPE.itemsize == 64

_MODES = {"boxes": _lib.VN_AUGMENT_BOXES, "rotate": _lib.VN_AUGMENT_ROTATE, "scale": _lib.VN_AUGMENT_SCALE}


@dataclass
class AugmentParams:
    """one sample's draw.  mode 'boxes': `table` holds the accepted perturbations in label order; 'rotate': `angle`;
    'scale': `factor`.  boxes_before / boxes_after: (G,7) float64 lidar boxes (x,y,z,h,w,l,r) of EVERY label line."""
    mode: str
    choice: int
    boxes_before: np.ndarray
    boxes_after: np.ndarray
    table: np.ndarray = field(default_factory=lambda: np.zeros(0, dtype=BOX_DTYPE))
    angle: float = 0.0
    factor: float = 1.0


def transform_box(box, tx, ty, tz, rz):
    """the rigid motion applied to one (7,) box: the centre moves like a point, h / w / l stay, r' = _limit_angle(r - rz)"""
    c, s = np.cos(rz), np.sin(rz)
    X, Y, Z = box[0] + tx, box[1] + ty, box[2] + tz
    out = np.array(box, dtype=np.float64)
    out[0] = X * c + Y * s
    out[1] = -(X * s) + Y * c
    out[2] = Z
    out[6] = _limit_angle(box[6] - rz)
    return out


def footprints_overlap(a, b):
    """exact separating-axis test (float64) of the rotated footprints of two (7,) boxes: True iff they overlap with
    positive area (touching edges or corners do not count).  A footprint is the l x w rectangle about (x, y) turned by r,
    as in targets.gt_standup_boxes."""
    la, wa, lb, wb = abs(a[5]) / 2, abs(a[4]) / 2, abs(b[5]) / 2, abs(b[4]) / 2
    if la * wa == 0.0 or lb * wb == 0.0:
        return False
    dx, dy = b[0] - a[0], b[1] - a[1]
    ca, sa, cb, sb = np.cos(a[6]), np.sin(a[6]), np.cos(b[6]), np.sin(b[6])
    # the axes of a: (ca, sa) along l, (-sa, ca) along w; likewise for b
    cab, sab = ca * cb + sa * sb, sa * cb - ca * sb          # cos / sin of (ra - rb)
    for ux, uy, ra, rb in ((ca, sa, la, lb * abs(cab) + wb * abs(sab)), (-sa, ca, wa, lb * abs(sab) + wb * abs(cab)),
                           (cb, sb, la * abs(cab) + wa * abs(sab), lb), (-sb, cb, la * abs(sab) + wa * abs(cab), wb)):
        if abs(dx * ux + dy * uy) >= ra + rb:
            return False
    return True


def box_bounds(box):
    """(lo (3,), hi (3,)) float32: axis-aligned hull of the box's eight corners — float64 rotation, corners stored
    float32 (targets.gt_standup_boxes); z from float32(z) (the box bottom) to float32(z + h)"""
    x0, y0, x1, y1 = gt_standup_boxes(np.asarray(box, dtype=np.float64).reshape(1, 7))[0]
    return (np.array([x0, y0, np.float32(box[2])], dtype=np.float32),
            np.array([x1, y1, np.float32(box[2] + box[3])], dtype=np.float32))


def draw_augmentation(labels):
    """labels: one sample's KITTI label lines.  Draws from the global np.random state (dataset.py:122-219):
    choice = randint(0, 10); >= 7 box perturbation (per box, up to 100 attempts of rz = uniform(-pi/10, pi/10), then
    tx, ty, tz = normal() each; the first attempt whose footprint overlaps no earlier — already moved — box is taken);
    4..6 global rotation by uniform(-pi/4, pi/4); < 4 global scaling by uniform(0.95, 1.05).  -> AugmentParams"""
    choice = int(np.random.randint(0, 10))
    before = label_to_gt_box_3d([labels], "", "lidar")[0]          # every line, all classes
    boxes = before.copy()
    if choice >= 7:
        rows = []
        for idx in range(boxes.shape[0]):
            for _ in range(MAX_ATTEMPTS):
                rz = np.random.uniform(-np.pi / 10, np.pi / 10)
                tx, ty, tz = np.random.normal(), np.random.normal(), np.random.normal()
                cand = transform_box(boxes[idx], tx, ty, tz, rz)
                if not any(footprints_overlap(cand, boxes[idy]) for idy in range(idx)):
                    lo, hi = box_bounds(boxes[idx])
                    rows.append((lo, hi, (tx, ty, tz), np.cos(rz), np.sin(rz)))
                    boxes[idx] = cand
                    break
        if len(rows) > MAX_BOXES:
            raise _lib.VoxelnetHipError(f"{len(rows)} perturbed boxes in one sample; vn_augment_points takes at most {MAX_BOXES}")
        table = np.zeros(len(rows), dtype=BOX_DTYPE)
        for i, row in enumerate(rows):
            table[i] = row
        return AugmentParams("boxes", choice, before, boxes, table=table)
    if choice >= 4:
        angle = float(np.random.uniform(-np.pi / 4, np.pi / 4))
        for idx in range(boxes.shape[0]):
            boxes[idx] = transform_box(boxes[idx], 0.0, 0.0, 0.0, angle)
        return AugmentParams("rotate", choice, before, boxes, angle=angle)
    factor = float(np.random.uniform(0.95, 1.05))
    boxes[:, 0:6] *= factor
    return AugmentParams("scale", choice, before, boxes, factor=factor)


def augment_labels(labels, params):
    """the sample's label lines after the draw, in label order: every line keeps its own class name, the box is
    params.boxes_after's in the format of targets.lidar_box_to_label_line (camera coordinates by the mean calibration,
    two decimals, the other fields zero — the target generator reads the class and the last seven fields only)"""
    if len(labels) != params.boxes_after.shape[0]:
        raise ValueError("params were drawn for another label")
    return [lidar_box_to_label_line(line.split()[0], box) for line, box in zip(labels, params.boxes_after)]


def enqueue_augment_points(points, params, out=None):
    """-> (out, tensors the queued work reads: keep them referenced until the stream has run it)"""
    if not (torch.is_tensor(points) and points.is_cuda and points.dtype == torch.float32 and points.dim() == 2
            and points.shape[1] == 4 and points.is_contiguous()):
        raise _lib.VoxelnetHipError("augment_points_device needs a contiguous (N,4) float32 HIP tensor (there is no CPU path)")
    if out is None:
        out = torch.empty_like(points)
    elif not (torch.is_tensor(out) and out.is_cuda and out.dtype == torch.float32 and out.shape == points.shape
              and out.is_contiguous() and out.device == points.device):
        raise _lib.VoxelnetHipError("augment_points_device: out must be a contiguous float32 HIP tensor of the points' shape")
    dev = points.device
    n = points.shape[0]
    keep = (points,)
    with _lib.on_device(dev):
        table_ptr, n_boxes, c, s, scale = None, 0, 1.0, 0.0, 1.0
        if params.mode == "boxes":
            n_boxes = int(params.table.shape[0])
            if n_boxes > MAX_BOXES:
                raise _lib.VoxelnetHipError(f"{n_boxes} table entries; vn_augment_points takes at most {MAX_BOXES}")
            if n_boxes:
                # pinned staging + an asynchronous copy on the current stream (as targets.TargetGenerator.from_boxes): a
                # copy from pageable memory would make the host wait for everything queued in front of it
                host = torch.from_numpy(np.ascontiguousarray(params.table, dtype=BOX_DTYPE).view(np.uint8)).pin_memory()
                table = host.to(dev, non_blocking=True)
                table_ptr = table.data_ptr()
                keep += (host, table)
        elif params.mode == "rotate":
            c, s = float(np.cos(params.angle)), float(np.sin(params.angle))
        elif params.mode == "scale":
            scale = float(np.float32(params.factor))
        else:
            raise ValueError(f"unknown augmentation mode {params.mode!r}")
        _lib.call("vn_augment_points", points.data_ptr(), n, _MODES[params.mode], table_ptr, n_boxes, c, s, scale,
                  out.data_ptr(), _lib.raw_stream())
    return out, keep


def augment_points_device(points, params, out=None):
    """points: contiguous (N,4) float32 HIP tensor [x,y,z,reflectance] -> the augmented cloud (`out`; a new tensor when
    None; `out=points` works in place), enqueued on the current stream without any host synchronisation.  Reflectance
    is never touched; NaN rows (the padded field-of-view crop) stay NaN.  Raises VoxelnetHipError for anything but a HIP
    tensor: the per-point work has no CPU path."""
    return enqueue_augment_points(points, params, out)[0]


# ---------------------------------------------------------------------------------------------------------------------
# the composed recipe: object noise -> flip -> rotation -> scaling -> translation, one launch (vn_augment_compose)
# ---------------------------------------------------------------------------------------------------------------------
# one entry of the device move table: vnObjectMove (include/voxelnet_hip.h), 128 bytes of float64 — the UNMOVED box in
# gtsample.BOX_DTYPE's fields, the object's translation, cos / sin of its turn about its own centre
MOVE_DTYPE = np.dtype([(n, "<f8") for n in ("x", "y", "z0", "z1", "hl", "hw", "c", "s", "tx", "ty", "tz", "rc", "rs")]
                      + [("pad", "<f8", 3)])
assert MOVE_DTYPE.itemsize == 128
AFFINE_FIELDS = ("a00", "a01", "a10", "a11", "sz", "bx", "by", "bz")          # vnAffine, in the header's order


@dataclass
class ComposeRecipe:
    """the composed augmentation; the defaults are the common KITTI recipe.  A stage set to None (flip: None or 0) is
    off and consumes NO random numbers.  Object noise is ONE stage: off when `attempts` is None / 0 or when object_rot
    and object_sigma are both None; with one of the two None that half is zero and every candidate still draws its
    four numbers.
      object_rot      : each object turns about its own centre by uniform(-object_rot, object_rot)
      object_sigma    : ... and moves by normal() * object_sigma per axis (x, y, z)
      attempts        : candidates per object before it is left where it is
      flip            : probability of y -> -y
      rotation        : global rotation by uniform(-rotation, rotation) about the lidar origin
      scale           : global scaling by uniform(*scale)
      translate_sigma : global translation by normal() * translate_sigma per axis"""
    object_rot: Optional[float] = np.pi / 4
    object_sigma: Optional[Tuple[float, float, float]] = (1.0, 1.0, 0.5)
    attempts: Optional[int] = 100
    flip: Optional[float] = 0.5
    rotation: Optional[float] = np.pi / 4
    scale: Optional[Tuple[float, float]] = (0.95, 1.05)
    translate_sigma: Optional[Tuple[float, float, float]] = None


@dataclass
class ComposeParams:
    """one sample's draw.  boxes_before / boxes_after: (G,7) float64 lidar boxes of EVERY label line (a DontCare line's
    row is the same in both); has_box: (G,) bool, False for DontCare lines; table: the accepted object moves in label
    order, entry_line[k] = the label line of entry k; flip_y, angle, factor (as drawn; the points use
    float(np.float32(factor))), translate: the global stages; affine: (8,) float64, vnAffine's fields in order."""
    boxes_before: np.ndarray
    boxes_after: np.ndarray
    has_box: np.ndarray
    table: np.ndarray
    entry_line: list
    flip_y: bool
    angle: float
    factor: float
    translate: tuple
    affine: np.ndarray


def compose_affine(flip_y, angle, factor, translate):
    """stages 2-5 as one vnAffine, float64, exactly:
        fy = -1.0 if flip_y else 1.0;  c, s = np.cos(angle), np.sin(angle)  (1.0, 0.0 when the rotation is off)
        f = float(np.float32(factor))  (1.0 when the scaling is off);  t = translate  ((0.0, 0.0, 0.0) when off)
        a00 = f * c      a01 = f * (s * fy)      a10 = f * (-s)      a11 = f * (c * fy)      sz = f      bx, by, bz = t
    i.e. (x, y) -> (x, fy*y) -> (X*c + Y*s, -(X*s) + Y*c) -> times f -> plus t.  -> (8,) float64 in AFFINE_FIELDS order"""
    fy = -1.0 if flip_y else 1.0
    c, s = (np.cos(angle), np.sin(angle)) if angle is not None else (1.0, 0.0)
    f = float(np.float32(factor)) if factor is not None else 1.0
    t = translate if translate is not None else (0.0, 0.0, 0.0)
    return np.array([f * c, f * (s * fy), f * (-s), f * (c * fy), f, t[0], t[1], t[2]], dtype=np.float64)


def draw_compose(labels, recipe):
    """labels: one sample's KITTI label lines; recipe: a ComposeRecipe.  Draws from the global np.random state, in this
    fixed order (a stage that is off draws nothing):
      1. object noise — for each line that has a 3D box (every type but DontCare), in label order, up to `attempts`
         candidates: rz = uniform(-object_rot, object_rot), then three normal() scaled by object_sigma.  The candidate —
         centre moved by t, r' = _limit_angle(r + rz) — is taken when its footprint overlaps (footprints_overlap) NO OTHER
         box with a 3D box in its current state: earlier ones moved, later ones unmoved.  No free candidate: the box
         stays and gets no table entry.
      2. flip       — flip_y = random() < flip.                  boxes: y -> -y, r -> -r
      3. rotation   — angle = uniform(-rotation, rotation).      boxes: x' = X*c + Y*s, y' = -(X*s) + Y*c, r' = r - angle
      4. scaling    — factor = uniform(*scale).                  boxes: [:, 0:6] *= factor
      5. translation— three normal() scaled by translate_sigma.  boxes: [:, 0:3] += t
    DontCare lines take no part.  -> ComposeParams"""
    from .gtsample import box_table
    before = label_to_gt_box_3d([labels], "", "lidar")[0]
    has_box = np.array([line.split()[0] != "DontCare" for line in labels], dtype=bool)
    boxes = before.copy()
    real = [int(i) for i in np.flatnonzero(has_box)]
    rows, entry_line = [], []
    if recipe.attempts and (recipe.object_rot is not None or recipe.object_sigma is not None):
        rot = 0.0 if recipe.object_rot is None else recipe.object_rot
        sig = (0.0, 0.0, 0.0) if recipe.object_sigma is None else recipe.object_sigma
        for idx in real:
            for _ in range(int(recipe.attempts)):
                rz = np.random.uniform(-rot, rot)
                tx, ty, tz = np.random.normal() * sig[0], np.random.normal() * sig[1], np.random.normal() * sig[2]
                cand = boxes[idx].copy()
                cand[0], cand[1], cand[2] = cand[0] + tx, cand[1] + ty, cand[2] + tz
                cand[6] = _limit_angle(cand[6] + rz)
                if not any(footprints_overlap(cand, boxes[idy]) for idy in real if idy != idx):
                    rows.append((box_table(before[idx])[0], tx, ty, tz, np.cos(rz), np.sin(rz)))
                    entry_line.append(idx)
                    boxes[idx] = cand
                    break
    if len(rows) > MAX_BOXES:
        raise _lib.VoxelnetHipError(f"{len(rows)} moved objects in one sample; vn_augment_compose takes at most {MAX_BOXES}")
    table = np.zeros(len(rows), dtype=MOVE_DTYPE)
    for i, (unmoved, tx, ty, tz, rc, rs) in enumerate(rows):
        for name in unmoved.dtype.names:
            table[i][name] = unmoved[name]
        table[i]["tx"], table[i]["ty"], table[i]["tz"], table[i]["rc"], table[i]["rs"] = tx, ty, tz, rc, rs
    flip_y, angle, factor, translate = False, None, None, None
    if recipe.flip:
        flip_y = bool(np.random.random() < recipe.flip)
        if flip_y:
            boxes[has_box, 1] = -boxes[has_box, 1]
            boxes[has_box, 6] = -boxes[has_box, 6]
    if recipe.rotation is not None:
        angle = float(np.random.uniform(-recipe.rotation, recipe.rotation))
        c, s = np.cos(angle), np.sin(angle)
        for idx in real:
            X, Y = boxes[idx, 0], boxes[idx, 1]
            boxes[idx, 0], boxes[idx, 1], boxes[idx, 6] = X * c + Y * s, -(X * s) + Y * c, boxes[idx, 6] - angle
    if recipe.scale is not None:
        factor = float(np.random.uniform(*recipe.scale))
        boxes[has_box, 0:6] *= factor
    if recipe.translate_sigma is not None:
        translate = tuple(float(np.random.normal() * sg) for sg in recipe.translate_sigma)
        boxes[has_box, 0:3] += np.array(translate)
    return ComposeParams(before, boxes, has_box, table, entry_line, flip_y, 0.0 if angle is None else angle,
                         1.0 if factor is None else factor, (0.0, 0.0, 0.0) if translate is None else translate,
                         compose_affine(flip_y, angle, factor, translate))


def compose_labels(labels, params):
    """the sample's label lines after the composed draw, in label order (the analogue of augment_labels): a line with a 3D
    box keeps its class name and carries params.boxes_after's box in the format of targets.lidar_box_to_label_line (two
    decimals); a DontCare line passes through verbatim"""
    if len(labels) != params.boxes_after.shape[0]:
        raise ValueError("params were drawn for another label")
    return [lidar_box_to_label_line(line.split()[0], box) if has else line
            for line, box, has in zip(labels, params.boxes_after, params.has_box)]


def enqueue_compose_points(points, params, out=None):
    """-> (out, tensors the queued work reads: keep them referenced until the stream has run it)"""
    if not (torch.is_tensor(points) and points.is_cuda and points.dtype == torch.float32 and points.dim() == 2
            and points.shape[1] == 4 and points.is_contiguous()):
        raise _lib.VoxelnetHipError("compose_points_device needs a contiguous (N,4) float32 HIP tensor (there is no CPU path)")
    if out is None:
        out = torch.empty_like(points)
    elif not (torch.is_tensor(out) and out.is_cuda and out.dtype == torch.float32 and out.shape == points.shape
              and out.is_contiguous() and out.device == points.device):
        raise _lib.VoxelnetHipError("compose_points_device: out must be a contiguous float32 HIP tensor of the points' shape")
    dev = points.device
    keep = (points,)
    table = np.ascontiguousarray(params.table, dtype=MOVE_DTYPE).reshape(-1)
    n_moves = int(table.shape[0])
    if n_moves > MAX_BOXES:
        raise _lib.VoxelnetHipError(f"{n_moves} table entries; vn_augment_compose takes at most {MAX_BOXES}")
    affine = _lib.VnAffine(*(float(v) for v in params.affine))          # read by the library at call time
    with _lib.on_device(dev):
        table_ptr = None
        if n_moves:
            # pinned staging + an asynchronous copy on the current stream, as enqueue_augment_points stages its table
            host = torch.from_numpy(table.view(np.uint8)).pin_memory()
            dev_table = host.to(dev, non_blocking=True)
            table_ptr = dev_table.data_ptr()
            keep += (host, dev_table)
        _lib.call("vn_augment_compose", points.data_ptr(), points.shape[0], table_ptr, n_moves, ctypes.byref(affine),
                  out.data_ptr(), _lib.raw_stream())
    return out, keep


def compose_points_device(points, params, out=None):
    """points: contiguous (N,4) float32 HIP tensor [x,y,z,reflectance] -> the cloud after the composed draw (`out`; a new
    tensor when None; `out=points` works in place), ONE launch enqueued on the current stream without any host
    synchronisation.  Reflectance is never touched; a NaN coordinate stays NaN.  Raises VoxelnetHipError for anything but a
    HIP tensor: the per-point work has no CPU path."""
    return enqueue_compose_points(points, params, out)[0]
