"""Ground-truth database sampling ("GT-paste", SECOND) as a stage of the input pipeline — the reference has no
counterpart.  Labelled objects are cut with their points out of the training frames once
(`GTDatabase`); every training frame then receives a few of them where they collide with nothing (`GTSampler`).  Split
where the work splits:

  host   (this module, O(boxes) NumPy): the draw, the collision test (`augment.footprints_overlap`), the table, the
         appended label lines
  device (csrc/gtsample.hip): the point-in-rotated-box test over N points x up to 128 boxes (`vn_points_in_boxes`) and
         the paste — drop the scene points inside the pasted boxes, keep the rest in order, append the objects' points,
         pad with NaN points (`vn_gt_paste`) — on the pipeline's stream between the field-of-view crop and the
         augmentation.  There is no CPU path for the points.

Table entry (vnGtBox, 64 bytes of float64) of a lidar box (x, y, z, h, w, l, r) in the convention of targets.py:
    x, y, z0 = z, z1 = z + h, hl = l / 2, hw = w / 2, c = cos(r), s = sin(r)            (NumPy's cos / sin, on the host)
Inside, for a float32 point widened exactly to float64, evaluated as written without contraction:
    dx = px - x;  dy = py - y;  u = dx*c + dy*s;  v = -(dx*s) + dy*c
    inside  <=>  |u| <= hl  and  |v| <= hw  and  pz >= z0  and  pz <= z1                  (inclusive; a NaN anywhere fails)

Objects are pasted at their source position: all frames share the lidar frame.  Stated divergences from SECOND: no
ground-plane alignment of a pasted object, no check that it is visible from the sensor (unless the sampler carries a
`Visibility`: below), the mean calibration as everywhere in targets.py, and pasted points come after all scene points (in
a voxel shared with surviving scene points the scene points win the T slots).

`GTSampler(..., visibility=Visibility())` switches the paste to `vn_gt_paste_visible`: a
coarse range image of the frame rejects objects hidden behind scene points, drops the hidden points of the others and
whatever lies in their shadow; `DeviceCollate` then drops the label lines of the rejected objects."""
import ctypes
import os
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from .augment import footprints_overlap
from .targets import label_to_gt_box_3d

MAX_BOXES = _lib.VN_GT_MAX_BOXES
# one entry of the device box table: vnGtBox (include/voxelnet_hip.h), 64 bytes
BOX_DTYPE = np.dtype([(n, "<f8") for n in ("x", "y", "z0", "z1", "hl", "hw", "c", "s")])
assert BOX_DTYPE.itemsize == 64


def box_table(boxes):
    """(G,7) float64 lidar boxes (x, y, z, h, w, l, r) -> (G,) BOX_DTYPE table"""
    b = np.asarray(boxes, dtype=np.float64).reshape(-1, 7)
    t = np.zeros(b.shape[0], dtype=BOX_DTYPE)
    t["x"], t["y"] = b[:, 0], b[:, 1]
    t["z0"], t["z1"] = b[:, 2], b[:, 2] + b[:, 3]
    t["hl"], t["hw"] = b[:, 5] / 2, b[:, 4] / 2
    t["c"], t["s"] = np.cos(b[:, 6]), np.sin(b[:, 6])
    return t


def _check_points(points, what):
    if not (torch.is_tensor(points) and points.is_cuda and points.dtype == torch.float32 and points.dim() == 2
            and points.shape[1] == 4 and points.is_contiguous()):
        raise _lib.VoxelnetHipError(f"{what} needs a contiguous (N,4) float32 HIP tensor (there is no CPU path)")


def _stage_table(table, dev, what):
    """-> (device pointer or None, entries, tensors to keep referenced): pinned staging + an asynchronous copy on the
    current stream, as augment.enqueue_augment_points stages its table"""
    table = np.ascontiguousarray(table, dtype=BOX_DTYPE).reshape(-1)
    g = int(table.shape[0])
    if g > MAX_BOXES:
        raise _lib.VoxelnetHipError(f"{g} table entries; {what} takes at most {MAX_BOXES}")
    if g == 0:
        return None, 0, ()
    host = torch.from_numpy(table.view(np.uint8)).pin_memory()
    dev_table = host.to(dev, non_blocking=True)
    return dev_table.data_ptr(), g, (host, dev_table)


def points_in_boxes_device(points, table, counts=True):
    """points: contiguous (N,4) float32 HIP tensor; table: (G <= 128,) BOX_DTYPE (box_table).  -> (index (N,) int32: the
    lowest table entry whose box holds the point, else -1; counts (G,) int32: points inside each box, a point inside two
    boxes counted for both — None with counts=False), device tensors, enqueued on the current stream."""
    _check_points(points, "points_in_boxes_device")
    dev, n = points.device, points.shape[0]
    with _lib.on_device(dev):
        ptr, g, keep = _stage_table(table, dev, "vn_points_in_boxes")
        index = torch.empty(n, dtype=torch.int32, device=dev)
        cnt = torch.empty(g, dtype=torch.int32, device=dev) if counts else None
        _lib.call("vn_points_in_boxes", points.data_ptr(), n, ptr, g, index.data_ptr(),
                  cnt.data_ptr() if counts and g else None, _lib.raw_stream())
    return index, cnt


@dataclass
class GTEntry:
    """one database object: its class, the tag of the frame it was cut from, its (7,) float64 lidar box, its (P,4)
    float32 points in the source cloud's order and its source label line, verbatim"""
    cls: str
    tag: str
    box: np.ndarray
    points: np.ndarray
    line: str


class GTDatabase:
    def __init__(self, entries=()):
        self.entries = list(entries)

    def __len__(self):
        return len(self.entries)

    def __getitem__(self, i):
        return self.entries[i]

    @classmethod
    def build(cls, frames, device="cuda:0", classes=("Car",)):
        """frames: iterable of (tag, cloud, label lines); the cloud — (N,4) float32, a NumPy array or a HIP tensor — is
        the one the model trains on (for raw sweeps: the cloud after fov_crop_device).  Every line whose type is exactly
        one of `classes` gives one entry: box = label_to_gt_box_3d([[line]], "", "lidar")[0][0], points = the cloud's
        rows inside that box in cloud order (overlapping boxes each keep their points; entries with 0 points are
        stored).  One vn_points_in_boxes launch per frame; a box that shares points with another one is cut with a
        launch of its own."""
        device = torch.device(device)
        if device.type != "cuda":
            raise _lib.VoxelnetHipError("GTDatabase.build needs a HIP device (there is no CPU path for the points)")
        classes = tuple(classes)
        entries = []
        for tag, cloud, labels in frames:
            lines = [line for line in labels if line.split() and line.split()[0] in classes]
            if not lines:
                continue
            if len(lines) > MAX_BOXES:
                raise _lib.VoxelnetHipError(f"{len(lines)} objects in frame {tag}; vn_points_in_boxes takes at most {MAX_BOXES}")
            boxes = np.stack([label_to_gt_box_3d([[line]], "", "lidar")[0][0] for line in lines])
            if torch.is_tensor(cloud):
                pts = cloud.to(device).contiguous()
            else:
                pts = torch.from_numpy(np.array(cloud, dtype=np.float32)).to(device)
            table = box_table(boxes)
            index, counts = points_in_boxes_device(pts, table)
            host, index, counts = pts.cpu().numpy(), index.cpu().numpy(), counts.cpu().numpy()
            for j, line in enumerate(lines):
                mask = index == j
                if int(mask.sum()) != int(counts[j]):          # some of its points also lie in an earlier box
                    mask = points_in_boxes_device(pts, table[j:j + 1], counts=False)[0].cpu().numpy() == 0
                entries.append(GTEntry(line.split()[0], str(tag), boxes[j].copy(), host[mask].copy(), line))
        return cls(entries)

    @classmethod
    def build_from_dataset(cls, dataset, device="cuda:0", classes=("Car",), fov_calib_dir=None, image_shape=(375, 1242)):
        """every sample (tag, img, pcl, labels, _) of a KITTIDataset-like dataset; fov_calib_dir: raw sweeps — each cloud
        is cropped to the camera field of view on the device first, as DeviceCollate(fov_calib_dir=...) does"""
        device = torch.device(device)
        if device.type != "cuda":
            raise _lib.VoxelnetHipError("GTDatabase.build_from_dataset needs a HIP device (there is no CPU path for the points)")

        def frames():
            for i in range(len(dataset)):
                tag, img, pcl, labels = dataset[i][:4]
                pts = torch.from_numpy(np.ascontiguousarray(pcl[:, :4], dtype=np.float32)).to(device)
                if fov_calib_dir is not None:
                    from .fov import fov_crop_device, load_calib
                    P, Tr, R = load_calib(os.path.join(fov_calib_dir, str(tag) + ".txt"))
                    rows, cols = img.shape[:2] if img is not None else tuple(image_shape)
                    pts = fov_crop_device(pts, P, Tr, R, rows, cols)
                yield tag, pts, labels
        return cls.build(frames(), device, classes)

    def save(self, path):
        """one .npz: concatenated points, offsets, boxes, class / tag / line arrays"""
        pts = [e.points for e in self.entries]
        offsets = np.zeros(len(pts) + 1, dtype=np.int64)
        offsets[1:] = np.cumsum([p.shape[0] for p in pts])
        with open(path, "wb") as fh:
            np.savez(fh, points=np.concatenate(pts + [np.zeros((0, 4), np.float32)]).astype(np.float32, copy=False),
                     offsets=offsets, boxes=np.array([e.box for e in self.entries], dtype=np.float64).reshape(-1, 7),
                     cls=np.array([e.cls for e in self.entries], dtype=np.str_),
                     tag=np.array([e.tag for e in self.entries], dtype=np.str_),
                     line=np.array([e.line for e in self.entries], dtype=np.str_))

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            pts, off, boxes = z["points"], z["offsets"], z["boxes"]
            return cls([GTEntry(str(c), str(t), boxes[i].copy(), pts[off[i]:off[i + 1]].copy(), str(line))
                        for i, (c, t, line) in enumerate(zip(z["cls"], z["tag"], z["line"]))])


@dataclass
class GTSampleParams:
    """one frame's draw, in acceptance order: `table` (G,) BOX_DTYPE, `points` (M,4) float32 = the accepted objects'
    points concatenated, `boxes` (G,7) float64, `lines` = their stored label lines (the frame's labels become
    labels + lines), `offsets` (G+1,) int32 = object o owns points[offsets[o]:offsets[o+1]] (GTSampler.draw fills it;
    only the visibility paste reads it)"""
    table: np.ndarray
    points: np.ndarray
    boxes: np.ndarray
    lines: list
    offsets: np.ndarray = None


@dataclass(frozen=True)
class Visibility:
    """the range image of the occlusion-consistent paste (vnVisGrid): four side faces of a cube
    around the sensor, `nu` bins across a face and `nv` rows over v = z / max(|x|, |y|) in [v_lo, v_hi); a point lies
    behind another one when its depth exceeds the other's by more than `margin` metres (inf: never); a pasted object
    needs `min_visible` visible points.  The defaults are about one HDL-64 beam per row and are not tuned."""
    nu: int = 512
    nv: int = 64
    v_lo: float = -0.47
    v_hi: float = 0.10
    margin: float = 0.3
    min_visible: int = 5

    def __post_init__(self):
        for name in ("nu", "nv", "min_visible"):
            v = getattr(self, name)
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"Visibility.{name}={v!r}: expected an integer")
            object.__setattr__(self, name, int(v))
        for name in ("v_lo", "v_hi", "margin"):
            object.__setattr__(self, name, float(getattr(self, name)))
        if not (2 <= self.nu <= 2048 and self.nu % 2 == 0):
            raise ValueError(f"Visibility.nu={self.nu}: expected an even number in 2..2048")
        if not 1 <= self.nv <= 256:
            raise ValueError(f"Visibility.nv={self.nv}: expected 1..256")
        if not (np.isfinite(self.v_lo) and np.isfinite(self.v_hi) and self.v_lo < self.v_hi):
            raise ValueError(f"Visibility.v_lo={self.v_lo}, v_hi={self.v_hi}: expected finite v_lo < v_hi")
        if not self.margin >= 0.0:                                   # (NaN fails; inf passes)
            raise ValueError(f"Visibility.margin={self.margin}: expected >= 0 (inf allowed)")
        if not 0 <= self.min_visible < 2 ** 31:
            raise ValueError(f"Visibility.min_visible={self.min_visible}: expected 0..2^31-1")
        if not (np.isfinite(self.v_scale) and self.v_scale > 0.0):
            raise ValueError(f"Visibility: nv / (v_hi - v_lo) = {self.v_scale} is not a positive finite number")

    @property
    def v_scale(self):
        return float(np.float64(self.nv) / (np.float64(self.v_hi) - np.float64(self.v_lo)))

    def grid(self):
        """-> the vnVisGrid the library reads during the call"""
        return _lib.VnVisGrid(self.nu, self.nv, self.v_lo, self.v_hi, self.v_scale, self.margin, self.min_visible, 0)


class GTSampler:
    def __init__(self, db, per_class=None, min_points=5, visibility=None):
        """per_class: {class: the number of objects of that class a frame is filled up to}, drawn in its order.
        visibility: a `Visibility` — DeviceCollate then pastes with vn_gt_paste_visible and drops the label lines of the
        objects it rejects; the draw itself is the same, random numbers included.  None: the plain paste."""
        if visibility is not None and not isinstance(visibility, Visibility):
            raise ValueError(f"visibility={visibility!r}: expected None or a gtsample.Visibility")
        self.visibility = visibility
        self.db = db
        self.per_class = dict(per_class if per_class is not None else {"Car": 15})
        self.min_points = int(min_points)
        self._pools = {c: [i for i, e in enumerate(db.entries) if e.cls == c and e.points.shape[0] >= self.min_points]
                       for c in self.per_class}

    def draw(self, labels, tag):
        """labels: the frame's label lines; tag: the frame's (its own objects are never drawn).  From the global
        np.random state, per class in per_class order: want = max(0, per_class[cls] - #lines of that type); pool = the
        class's entries with >= min_points points and another tag, in database order; when want == 0 or the pool is
        empty NO random number is consumed, else exactly one np.random.permutation(len(pool)), whose first `want` are
        the candidates.  A candidate is accepted when its footprint overlaps no box of the frame (every line, DontCare
        included) and no candidate accepted earlier, of any class; at most 128 in total.  -> GTSampleParams"""
        existing = label_to_gt_box_3d([labels], "", "lidar")[0]
        entries, tag, taken = self.db.entries, str(tag), []
        for c, target in self.per_class.items():
            want = max(0, int(target) - sum(1 for line in labels if line.split() and line.split()[0] == c))
            pool = [i for i in self._pools[c] if entries[i].tag != tag]
            if want == 0 or not pool:
                continue
            for j in np.random.permutation(len(pool))[:want]:
                if len(taken) >= MAX_BOXES:
                    break
                cand = entries[pool[j]]
                if any(footprints_overlap(cand.box, b) for b in existing) or \
                        any(footprints_overlap(cand.box, t.box) for t in taken):
                    continue
                taken.append(cand)
        boxes = np.array([e.box for e in taken], dtype=np.float64).reshape(-1, 7)
        points = np.concatenate([e.points for e in taken] + [np.zeros((0, 4), np.float32)]).astype(np.float32, copy=False)
        offsets = np.zeros(len(taken) + 1, dtype=np.int32)
        offsets[1:] = np.cumsum([e.points.shape[0] for e in taken], dtype=np.int64)
        return GTSampleParams(box_table(boxes), points, boxes, [e.line for e in taken], offsets)


def _paste(points, params, cap):
    _check_points(points, "gt_paste_device")
    dev, n = points.device, points.shape[0]
    obj_host = np.array(params.points, dtype=np.float32).reshape(-1, 4)          # (a copy: the staging needs a writable array)
    m = int(obj_host.shape[0])
    cap = n + m if cap is None else int(cap)
    keep = (points,)
    with _lib.on_device(dev):
        ptr, g, staged = _stage_table(params.table, dev, "vn_gt_paste")
        keep += staged
        obj_ptr = None
        if m:
            host = torch.from_numpy(obj_host).pin_memory()
            obj = host.to(dev, non_blocking=True)
            obj_ptr = obj.data_ptr()
            keep += (host, obj)
        out = torch.empty((max(cap, 1), 4), dtype=torch.float32, device=dev)
        count = torch.empty(1, dtype=torch.int32, device=dev)
        nbytes = _lib.load().vn_gt_paste_workspace_bytes(n)
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
        _lib.call("vn_gt_paste", points.data_ptr(), n, ptr, g, obj_ptr, m, out.data_ptr(), cap, count.data_ptr(),
                  ws.data_ptr(), ws.numel(), _lib.raw_stream())
    return out[:max(cap, 0)], count, keep + (count, ws)


def enqueue_gt_paste(points, params, cap=None):
    """-> (out: the capacity-sized (cap = N + M by default, 4) buffer — kept scene rows in order, the objects' points,
    NaN points —, tensors the queued work reads: keep them referenced until the stream has run it).  No host
    synchronisation: the voxelizer drops the NaN rows like any out-of-range point."""
    out, _, keep = _paste(points, params, cap)
    return out, keep


def gt_paste_device(points, params, padded=False, cap=None):
    """points: contiguous (N,4) float32 HIP tensor -> the pasted cloud: the scene rows that are not NaN points and lie in
    none of params' boxes, in input order, then params.points (a view of the capacity-sized buffer sliced to the count:
    one device->host read of 4 bytes).  padded=True: no host synchronisation — (the whole buffer, whose rows past the
    count are NaN points; the count as a device int32 tensor).  Raises VoxelnetHipError for anything but a HIP tensor."""
    out, count, _ = _paste(points, params, cap)
    if padded:
        return out, count
    return out[:int(count.item())]


class GTVisibleResult:
    """what vn_gt_paste_visible reports besides the cloud, held on the device until it is read: `visible` (G,) int32 =
    the visible points per object, `accepted` (G,) bool = visible >= min_visible, `kept` (G,) int32 = the points per
    object in the output, `stats` (2,) int32 = scene rows removed by an accepted box / by shadow only.  Each attribute is a
    NumPy array read back from the device (a host synchronisation) when it is asked for."""

    def __init__(self, visible, kept, stats, min_visible):
        self._visible, self._kept, self._stats, self.min_visible = visible, kept, stats, int(min_visible)

    @property
    def visible(self):
        return self._visible.cpu().numpy()

    @property
    def visible_device(self):
        """the (G,) int32 device tensor itself: no synchronisation"""
        return self._visible

    @property
    def kept(self):
        return self._kept.cpu().numpy()

    @property
    def stats(self):
        return self._stats.cpu().numpy()

    @property
    def accepted(self):
        return self.visible >= self.min_visible


def _paste_visible(points, params, visibility, cap):
    _check_points(points, "gt_paste_visible_device")
    if not isinstance(visibility, Visibility):
        raise ValueError(f"visibility={visibility!r}: expected a gtsample.Visibility")
    dev, n = points.device, points.shape[0]
    obj_host = np.array(params.points, dtype=np.float32).reshape(-1, 4)          # (a copy: the staging needs a writable array)
    m = int(obj_host.shape[0])
    if params.offsets is None:
        raise _lib.VoxelnetHipError("vn_gt_paste_visible needs params.offsets (GTSampler.draw fills it)")
    offsets = np.ascontiguousarray(params.offsets, dtype=np.int32).reshape(-1)   # host memory, read during the call
    cap = n + m if cap is None else int(cap)
    keep = (points,)
    with _lib.on_device(dev):
        ptr, g, staged = _stage_table(params.table, dev, "vn_gt_paste_visible")
        if offsets.shape[0] != g + 1:
            raise _lib.VoxelnetHipError(f"{offsets.shape[0]} offsets for {g} table entries; vn_gt_paste_visible needs {g + 1}")
        keep += staged
        obj_ptr = None
        if m:
            host = torch.from_numpy(obj_host).pin_memory()
            obj = host.to(dev, non_blocking=True)
            obj_ptr = obj.data_ptr()
            keep += (host, obj)
        out = torch.empty((max(cap, 1), 4), dtype=torch.float32, device=dev)
        # count | stats[2] | visible[g] | kept[g]: one allocation, every slice 4-byte aligned
        ints = torch.empty(3 + 2 * g, dtype=torch.int32, device=dev)
        count, stats, visible, kept = ints[0:1], ints[1:3], ints[3:3 + g], ints[3 + g:3 + 2 * g]
        grid = visibility.grid()
        nbytes = _lib.load().vn_gt_paste_visible_workspace_bytes(n, m, ctypes.byref(grid))
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
        _lib.call("vn_gt_paste_visible", points.data_ptr(), n, ptr, g, obj_ptr, m, offsets.ctypes.data, ctypes.byref(grid),
                  out.data_ptr(), cap, count.data_ptr(), visible.data_ptr() if g else None, kept.data_ptr() if g else None,
                  stats.data_ptr(), ws.data_ptr(), ws.numel(), _lib.raw_stream())
    return out[:max(cap, 0)], count, GTVisibleResult(visible, kept, stats, visibility.min_visible), keep + (ints, ws)


def enqueue_gt_paste_visible(points, params, visibility, cap=None, return_result=False):
    """the occlusion-consistent paste without host synchronisation -> (out: the capacity-sized buffer of enqueue_gt_paste,
    tensors the queued work reads or writes: keep them referenced until the stream has run it, visible: a PINNED host
    (G,) int32 tensor — it is also among the kept references — into which a device->host copy of the visible counts is
    queued right behind the call: valid once the stream has run that copy; object o is accepted when visible[o] >=
    visibility.min_visible).  return_result=True: a fourth element, the call's GTVisibleResult — its `visible_device` is
    what a later stage on the same stream gates on (part_augment.enqueue_part_points)."""
    out, _, res, keep = _paste_visible(points, params, visibility, cap)
    with _lib.on_device(points.device):
        visible = torch.empty(res._visible.shape[0], dtype=torch.int32).pin_memory()
        visible.copy_(res._visible, non_blocking=True)
    if return_result:
        return out, keep + (visible,), visible, res
    return out, keep + (visible,), visible


def gt_paste_visible_device(points, params, visibility, padded=False, cap=None):
    """points: contiguous (N,4) float32 HIP tensor; params: a GTSampleParams with `offsets`; visibility: a Visibility ->
    (the pasted cloud, the count, a GTVisibleResult): the scene rows that are not NaN points, lie in no accepted object's
    box and in no accepted object's shadow, in input order, then the kept points of the accepted objects (a view of the
    capacity-sized buffer sliced to the count, which is then a Python int: one device->host read of 4 bytes).
    padded=True: no host synchronisation — the whole buffer, whose rows past the count are NaN points, and the count as a
    device int32 tensor.  Raises VoxelnetHipError for anything but a HIP tensor."""
    out, count, res, _ = _paste_visible(points, params, visibility, cap)
    if padded:
        return out, count, res
    k = int(count.item())
    return out[:k], k, res
