"""Part-aware object augmentation as a stage of the input pipeline — SE-SSD's "shape-aware" and PA-AUG's "part-aware"
augmentation; the reference has no counterpart.  An object's box is cut into the six
pyramids that join its centre to its faces (pyramid f = 2 * axis + (negative side ? 1 : 0); axis 0 = along the length,
1 = across it, 2 = up).  Per object one pyramid may lose all its points (drop: an occluded side), one may be thinned
(thin: a farther, sparser return) and one may be exchanged with the same pyramid of another object of its class,
rescaled to that object's box (swap).  With GT-paste on, most objects of a training frame are pasted copies that recur
over and over; this stage makes them differ.  Split where the work splits:

  host   (this module, O(boxes) NumPy): the draw, the pairing, the extent ratios, the table
  device (csrc/part_augment.hip, `vn_part_augment`): owner and pyramid of every point over N points x up to 128 boxes and
         the three operations, on the pipeline's stream between the paste and the augmentation.  There is no CPU path for
         the points.

Table entry (vnPartBox, 128 bytes) of a lidar box (x, y, z, h, w, l, r): gtsample.box_table's eight fields, then the
ratios ru, rv, rw = partner extent / own extent along the length, the width and the height, the three masks, the
partner's entry, the thinning key, threshold and minimum.  include/voxelnet_hip.h states the per-point rules.

Stated divergences from SE-SSD: thinning is a keyed Bernoulli draw per point (a hash of the row index) instead of
farthest-point sampling; an object takes at most one operation of each kind; removed rows become NaN points in place
instead of being compacted away (the voxelizer drops them like the padding rows of the field-of-view crop).

`DeviceCollate(..., part_augment=PartRecipe())` / `DeviceBatcher(..., part_augment=PartRecipe())` run it per sample."""
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from .gtsample import BOX_DTYPE, box_table
from .targets import label_to_gt_box_3d

MAX_BOXES = _lib.VN_PART_MAX_BOXES
FACES = 6
THRESH_ONE = 1 << 24          # sparse_thresh of "keep every row"
# one entry of the device table: vnPartBox (include/voxelnet_hip.h), 128 bytes
PART_DTYPE = np.dtype([(n, "<f8") for n in BOX_DTYPE.names + ("ru", "rv", "rw")]
                      + [(n, "<i4") for n in ("drop_mask", "sparse_mask", "swap_mask", "swap_with")]
                      + [("sparse_key", "<u4"), ("sparse_thresh", "<u4"), ("sparse_min", "<i4"), ("reserved", "<i4"), ("pad", "<f8")])
assert PART_DTYPE.itemsize == 128


@dataclass
class PartRecipe:
    """the part-aware draw.  A stage whose probability is None or 0 is off and consumes NO random numbers.
      drop_prob   : per object, the probability that one pyramid (uniform over the six) loses all its points
      sparse_prob : per object, the probability that one pyramid is thinned
      sparse_keep : the share of a thinned pyramid's points that stay (each point on its own, by a keyed hash)
      sparse_min  : a pyramid with fewer points than this is not thinned
      swap_prob   : per pair of objects of one class, the probability that they exchange one pyramid
    The defaults are not tuned: nobody has trained with them."""
    drop_prob: float = 0.25
    sparse_prob: float = 0.25
    sparse_keep: float = 0.5
    sparse_min: int = 16
    swap_prob: float = 0.25

    def __post_init__(self):
        for name in ("drop_prob", "sparse_prob", "swap_prob"):
            v = getattr(self, name)
            if v is None:
                continue
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) or not 0.0 <= v <= 1.0:
                raise ValueError(f"PartRecipe.{name}={v!r}: expected None or a probability in [0, 1]")
            setattr(self, name, float(v))
        v = self.sparse_keep
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) or not 0.0 <= v <= 1.0:
            raise ValueError(f"PartRecipe.sparse_keep={v!r}: expected a share in [0, 1]")
        self.sparse_keep = float(v)
        v = self.sparse_min
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or not 0 <= v < 2 ** 31:
            raise ValueError(f"PartRecipe.sparse_min={v!r}: expected an integer in 0..2^31-1")
        self.sparse_min = int(v)


@dataclass
class PartParams:
    """one sample's draw: `table` (G,) PART_DTYPE, one entry per label line that has a 3D box, in label order;
    entry_line[k] = the label line of entry k; `boxes` (G,7) float64 = the entries' lidar boxes"""
    table: np.ndarray
    entry_line: list
    boxes: np.ndarray


def part_table(boxes):
    """(G,7) float64 lidar boxes -> (G,) PART_DTYPE table on which nothing happens: the boxes, ratios 1, masks 0, no
    partner"""
    base = box_table(boxes)
    t = np.zeros(base.shape[0], dtype=PART_DTYPE)
    for name in BOX_DTYPE.names:
        t[name] = base[name]
    t["ru"] = t["rv"] = t["rw"] = 1.0
    t["swap_with"] = -1
    return t


def draw_parts(labels, recipe):
    """labels: one sample's KITTI label lines; recipe: a PartRecipe.  Every line that has a 3D box (every type but
    DontCare) gets one table entry, in label order; more than 128 raise VoxelnetHipError.  Draws from the global np.random
    state, stage by stage in this fixed order (a stage that is off draws nothing):
      1. drop — for each entry in order: random(); below drop_prob: f = randint(0, 6), drop_mask = 1 << f.
      2. thin — for each entry in order: random(); below sparse_prob: f = randint(0, 6), sparse_mask = 1 << f, then
         sparse_key = randint(0, 2**32, dtype=np.uint32); sparse_thresh = floor(sparse_keep * 2^24), sparse_min = the
         recipe's.
      3. swap — the types in order of first appearance; for each type with at least 2 entries one
         permutation(number of its entries), which orders them; for the consecutive pairs (first with second, third with
         fourth, ...; an odd last entry stays alone): random(); below swap_prob: f = randint(0, 6); both entries get
         swap_mask = 1 << f and each other's index, and ru, rv, rw = (partner's l / 2) / (own l / 2), likewise w / 2 and
         h / 2, in float64.  A pair with an extent that is not a positive finite number draws the same numbers and gets
         no swap.
    -> PartParams"""
    all_boxes = label_to_gt_box_3d([labels], "", "lidar")[0]
    lines = [i for i, line in enumerate(labels) if line.split()[0] != "DontCare"]
    if len(lines) > MAX_BOXES:
        raise _lib.VoxelnetHipError(f"{len(lines)} objects in one sample; vn_part_augment takes at most {MAX_BOXES}")
    boxes = np.asarray(all_boxes, dtype=np.float64).reshape(-1, 7)[lines]
    table = part_table(boxes)
    g = len(lines)
    if recipe.drop_prob:
        for k in range(g):
            if np.random.random() < recipe.drop_prob:
                table[k]["drop_mask"] = 1 << int(np.random.randint(0, FACES))
    if recipe.sparse_prob:
        for k in range(g):
            if np.random.random() < recipe.sparse_prob:
                table[k]["sparse_mask"] = 1 << int(np.random.randint(0, FACES))
                table[k]["sparse_key"] = np.random.randint(0, 2 ** 32, dtype=np.uint32)
                table[k]["sparse_thresh"] = int(np.floor(recipe.sparse_keep * THRESH_ONE))
                table[k]["sparse_min"] = recipe.sparse_min
    if recipe.swap_prob:
        by_type = {}
        for k, i in enumerate(lines):
            by_type.setdefault(labels[i].split()[0], []).append(k)          # (a dict keeps the order of first appearance)
        for members in by_type.values():
            if len(members) < 2:
                continue
            order = [members[j] for j in np.random.permutation(len(members))]
            for a, b in zip(order[0::2], order[1::2]):
                if not np.random.random() < recipe.swap_prob:
                    continue
                f = int(np.random.randint(0, FACES))
                ha, hb = boxes[a, [5, 4, 3]] / 2, boxes[b, [5, 4, 3]] / 2          # half length, width, height
                if not (np.isfinite(ha).all() and np.isfinite(hb).all() and (ha > 0).all() and (hb > 0).all()):
                    continue
                for own, other, h_own, h_other in ((a, b, ha, hb), (b, a, hb, ha)):
                    table[own]["swap_mask"], table[own]["swap_with"] = 1 << f, other
                    table[own]["ru"], table[own]["rv"], table[own]["rw"] = h_other / h_own
    return PartParams(table, lines, boxes)


class PartResult:
    """what vn_part_augment reports besides the cloud, held on the device until it is read: `counts` (G,6) int32 = the
    points per entry and pyramid before any operation, `stats` (G,3) int32 = the points per entry that were dropped /
    thinned away / moved to the partner.  Each attribute is a NumPy array read back from the device (a host
    synchronisation) when it is asked for."""

    def __init__(self, counts, stats):
        self._counts, self._stats = counts, stats

    @property
    def counts(self):
        return self._counts.cpu().numpy()

    @property
    def stats(self):
        return self._stats.cpu().numpy()


def check_table(table):
    """the host's check of a table before it is staged -> the (G,) PART_DTYPE array.  ValueError: a swap_with outside
    [-1, G), a sparse_thresh above 2^24, a negative sparse_min; VoxelnetHipError: more than 128 entries"""
    table = np.ascontiguousarray(table, dtype=PART_DTYPE).reshape(-1)
    g = int(table.shape[0])
    if g > MAX_BOXES:
        raise _lib.VoxelnetHipError(f"{g} table entries; vn_part_augment takes at most {MAX_BOXES}")
    if g and not ((table["swap_with"] >= -1) & (table["swap_with"] < g)).all():
        raise ValueError(f"swap_with outside [-1, {g}): {table['swap_with'].tolist()}")
    if g and (table["sparse_thresh"] > THRESH_ONE).any():
        raise ValueError(f"sparse_thresh above 2^24: {table['sparse_thresh'].tolist()}")
    if g and (table["sparse_min"] < 0).any():
        raise ValueError(f"negative sparse_min: {table['sparse_min'].tolist()}")
    return table


def enqueue_part_points(points, params, out=None, gate=None, gate_first=0, gate_min=0):
    """-> (out, tensors the queued work reads or writes: keep them referenced until the stream has run it, a PartResult).
    gate: None, or a contiguous int32 HIP tensor of G - gate_first values (the device `visible` counts of
    vn_gt_paste_visible): entry o >= gate_first takes part only when gate[o - gate_first] >= gate_min.  No host
    synchronisation."""
    table = check_table(params.table)
    if not (torch.is_tensor(points) and points.is_cuda and points.dtype == torch.float32 and points.dim() == 2
            and points.shape[1] == 4 and points.is_contiguous()):
        raise _lib.VoxelnetHipError("part_points_device needs a contiguous (N,4) float32 HIP tensor (there is no CPU path)")
    if out is None:
        out = torch.empty_like(points)
    elif not (torch.is_tensor(out) and out.is_cuda and out.dtype == torch.float32 and out.shape == points.shape
              and out.is_contiguous() and out.device == points.device):
        raise _lib.VoxelnetHipError("part_points_device: out must be a contiguous float32 HIP tensor of the points' shape")
    g =int(table.shape[0])
    gate_first, gate_min = int(gate_first), int(gate_min)
    if not 0 <= gate_first <= g:
        raise ValueError(f"gate_first={gate_first} outside [0, {g}]")
    if gate is not None:
        if not (torch.is_tensor(gate) and gate.is_cuda and gate.dtype == torch.int32 and gate.dim() == 1
                and gate.is_contiguous() and gate.device == points.device):
            raise _lib.VoxelnetHipError("part_points_device: gate must be a contiguous 1-D int32 HIP tensor on the points' device")
        if gate.shape[0] != g - gate_first:
            raise ValueError(f"{gate.shape[0]} gate values for entries {gate_first}..{g - 1}")
    dev, n = points.device, points.shape[0]
    keep = (points,) if gate is None else (points, gate)
    with _lib.on_device(dev):
        table_ptr = None
        if g:
            # pinned staging + an asynchronous copy on the current stream, as augment.enqueue_compose_points stages its table
            host = torch.from_numpy(table.view(np.uint8)).pin_memory()
            dev_table = host.to(dev, non_blocking=True)
            table_ptr = dev_table.data_ptr()
            keep += (host, dev_table)
        ints = torch.empty(g * (FACES + 3), dtype=torch.int32, device=dev)          # counts | stats: one allocation
        counts, stats = ints[:g * FACES].view(g, FACES), ints[g * FACES:].view(g, 3)
        nbytes = _lib.load().vn_part_augment_workspace_bytes(n, g)
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
        _lib.call("vn_part_augment", points.data_ptr(), n, table_ptr, g, gate.data_ptr() if gate is not None and g else None,
                  gate_first, gate_min, out.data_ptr(), counts.data_ptr() if g else None, stats.data_ptr() if g else None,
                  ws.data_ptr(), ws.numel(), _lib.raw_stream())
    return out, keep + (ints, ws), PartResult(counts, stats)


def part_points_device(points, params, out=None, gate=None, gate_first=0, gate_min=0):
    """points: contiguous (N,4) float32 HIP tensor [x,y,z,reflectance] -> (the cloud after the part-aware draw — `out`; a
    new tensor when None; `out=points` works in place —, a PartResult), three launches enqueued on the current stream
    without any host synchronisation.  Dropped and thinned rows become NaN points, which the voxelizer drops; every row
    that no rule touches keeps its bits.  Raises VoxelnetHipError for anything but a HIP tensor: the per-point work has no
    CPU path."""
    out, _, result = enqueue_part_points(points, params, out, gate, gate_first, gate_min)
    return out, result
