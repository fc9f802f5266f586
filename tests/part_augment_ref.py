"""NumPy restatement of the part-aware object augmentation (voxelnet_amd/part_augment.py's draw_parts +
csrc/part_augment.hip's vn_part_augment) — the arbiter of the device kernels and of the host draw.

Written on its own from the rules in include/voxelnet_hip.h, sharing with the package only targets.label_to_gt_box_3d for
the boxes and NumPy's cos / sin:
  - every float64 expression is elementwise and spelled exactly as the header writes it (no matmul: a BLAS may fuse a
    multiply and an add), rounded once to float32;
  - the owner is decided once, on the input cloud: the lowest LIVE entry whose box holds the point;
  - fmix32 is exact: uint64 arithmetic masked to 32 bits;
  - a table is a list of dicts (`entry()`), a gate a plain sequence of ints."""
import numpy as np

from voxelnet_amd.targets import label_to_gt_box_3d

FIELDS_F8 = ("x", "y", "z0", "z1", "hl", "hw", "c", "s", "ru", "rv", "rw")
FIELDS_INT = ("drop_mask", "sparse_mask", "swap_mask", "swap_with", "sparse_key", "sparse_thresh", "sparse_min")
QNAN = np.uint32(0x7FC00000)
M32 = np.uint64(0xFFFFFFFF)


def entry(box, drop=0, sparse=0, swap=0, swap_with=-1, key=0, thresh=0, min_points=0, ratios=(1.0, 1.0, 1.0)):
    """table entry of a (7,) lidar box (x, y, z, h, w, l, r): a dict; masks as integers (bit f = pyramid f)"""
    return dict(x=float(box[0]), y=float(box[1]), z0=float(box[2]), z1=float(box[2] + box[3]), hl=float(box[5] / 2),
                hw=float(box[4] / 2), c=float(np.cos(box[6])), s=float(np.sin(box[6])), ru=float(ratios[0]), rv=float(ratios[1]),
                rw=float(ratios[2]), drop_mask=int(drop), sparse_mask=int(sparse), swap_mask=int(swap), swap_with=int(swap_with),
                sparse_key=int(key), sparse_thresh=int(thresh), sparse_min=int(min_points))


def pair(table, a, b, boxes, f):
    """make entries a and b swap pyramid f: the mask, each other's index, the ratios of the half extents"""
    for own, other in ((a, b), (b, a)):
        table[own]["swap_mask"], table[own]["swap_with"] = 1 << f, other
        table[own]["ru"] = (boxes[other][5] / 2) / (boxes[own][5] / 2)
        table[own]["rv"] = (boxes[other][4] / 2) / (boxes[own][4] / 2)
        table[own]["rw"] = (boxes[other][3] / 2) / (boxes[own][3] / 2)


def fmix32(x):
    x = np.asarray(x, dtype=np.uint64) & M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x85EBCA6B)) & M32
    x ^= x >> np.uint64(13)
    x = (x * np.uint64(0xC2B2AE35)) & M32
    x ^= x >> np.uint64(16)
    return x


def live_entries(n_entries, gate=None, gate_first=0, gate_min=0):
    return [not (gate is not None and o >= gate_first and int(gate[o - gate_first]) < gate_min) for o in range(n_entries)]


def local(px, py, pz, e):
    """u, v, w of float64 coordinates in entry e's box"""
    with np.errstate(invalid="ignore"):
        dx, dy = px - e["x"], py - e["y"]
        u = dx * e["c"] + dy * e["s"]
        v = -(dx * e["s"]) + dy * e["c"]
        hh = (e["z1"] - e["z0"]) * 0.5
        w = pz - (e["z0"] + hh)
    return u, v, w


def inside(cloud, e):
    px, py, pz = (cloud[:, a].astype(np.float64) for a in range(3))
    u, v, _ = local(px, py, pz, e)
    with np.errstate(invalid="ignore"):
        return (np.abs(u) <= e["hl"]) & (np.abs(v) <= e["hw"]) & (pz >= e["z0"]) & (pz <= e["z1"])


def pyramid(u, v, w, e):
    hh = (e["z1"] - e["z0"]) * 0.5
    m0 = np.abs(u) * (e["hw"] * hh)
    m1 = np.abs(v) * (e["hl"] * hh)
    m2 = np.abs(w) * (e["hl"] * e["hw"])
    axis = np.where((m0 >= m1) & (m0 >= m2), 0, np.where(m1 >= m2, 1, 2))
    along = np.where(axis == 0, u, np.where(axis == 1, v, w))
    return 2 * axis + (along < 0)


def owner_face(cloud, table, gate=None, gate_first=0, gate_min=0):
    """-> (owner (N,) int: the lowest live entry that holds the row, else -1; face (N,) int: its pyramid, else -1)"""
    cloud = np.asarray(cloud, dtype=np.float32).reshape(-1, 4)
    alive = live_entries(len(table), gate, gate_first, gate_min)
    nan = np.isnan(cloud[:, :3]).any(1)
    own = np.full(len(cloud), -1, dtype=np.int64)
    for o in range(len(table) - 1, -1, -1):
        if alive[o]:
            own[inside(cloud, table[o]) & ~nan] = o
    face = np.full(len(cloud), -1, dtype=np.int64)
    for o, e in enumerate(table):
        m = own == o
        u, v, w = local(*(cloud[m, a].astype(np.float64) for a in range(3)), e)
        face[m] = pyramid(u, v, w, e)
    return own, face


def swap_xyz(u, v, w, e, p):
    """float64 position in partner p's box of local coordinates (u, v, w) of entry e's"""
    u2, v2, w2 = u * e["ru"], v * e["rv"], w * e["rw"]
    hh = (p["z1"] - p["z0"]) * 0.5
    return p["x"] + (u2 * p["c"] - v2 * p["s"]), p["y"] + (u2 * p["s"] + v2 * p["c"]), (p["z0"] + hh) + w2


def apply(cloud, table, gate=None, gate_first=0, gate_min=0):
    """cloud (N,4) float32 -> (out (N,4) float32, counts (G,6) int32, stats (G,3) int32)"""
    cloud = np.asarray(cloud, dtype=np.float32).reshape(-1, 4)
    g = len(table)
    alive = live_entries(g, gate, gate_first, gate_min)
    own, face = owner_face(cloud, table, gate, gate_first, gate_min)
    counts, stats = np.zeros((g, 6), dtype=np.int32), np.zeros((g, 3), dtype=np.int32)
    for o in range(g):
        counts[o] = np.bincount(face[own == o], minlength=6)
    out = cloud.copy()
    bits = out.view(np.uint32)
    for o, e in enumerate(table):
        rows = np.flatnonzero(own == o)
        f = face[rows]
        drop = (((e["drop_mask"] & 0x3F) >> f) & 1).astype(bool)
        h = fmix32(rows.astype(np.uint64) ^ np.uint64(e["sparse_key"])) >> np.uint64(8)
        thin = ~drop & (((e["sparse_mask"] & 0x3F) >> f) & 1).astype(bool) & (counts[o][f] >= e["sparse_min"]) & \
            (h >= np.uint64(e["sparse_thresh"]))
        p = e["swap_with"]
        partner = 0 <= p < g and p != o and alive[p]
        swap = ~drop & ~thin & (((e["swap_mask"] & 0x3F) >> f) & 1).astype(bool) & bool(partner)
        bits[rows[drop | thin]] = QNAN
        stats[o] = (drop.sum(), thin.sum(), swap.sum())
        r = rows[swap]
        if len(r):
            u, v, w = local(*(cloud[r, a].astype(np.float64) for a in range(3)), e)
            X, Y, Z = swap_xyz(u, v, w, e, table[p])
            with np.errstate(over="ignore", invalid="ignore"):
                out[r, 0], out[r, 1], out[r, 2] = X.astype(np.float32), Y.astype(np.float32), Z.astype(np.float32)
    return out, counts, stats


# ---------------------------------------------------------------------------------------------------------------------
# bridges to the package's types (tests only)
# ---------------------------------------------------------------------------------------------------------------------
def to_params(table):
    """entry() dicts -> the package's PartParams (no label lines: for the device wrappers only)"""
    from voxelnet_amd import part_augment as P
    t = np.zeros(len(table), dtype=P.PART_DTYPE)
    for i, e in enumerate(table):
        for n in FIELDS_F8 + FIELDS_INT:
            t[i][n] = e[n]
    return P.PartParams(t, [], np.zeros((len(table), 7)))


def from_params(params):
    """the package's PartParams -> entry() dicts, value for value"""
    return [{**{n: float(row[n]) for n in FIELDS_F8}, **{n: int(row[n]) for n in FIELDS_INT}} for row in params.table]


def same(a, b):
    """bit-equal float32 arrays (NaN rows: NaN in the same places — a NaN's payload is not part of the contract)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan]))


# ---------------------------------------------------------------------------------------------------------------------
# hand-picked edge points, with their owners and pyramids worked out by hand (pyramid f: 0 +u, 1 -u, 2 +v, 3 -v, 4 +w, 5 -w)
# ---------------------------------------------------------------------------------------------------------------------
BOX_A = np.array([0.0, 0.0, -0.5, 1.0, 2.0, 4.0, 0.0])          # r = 0 about the origin: u = x, v = y, w = z; hl 2, hw 1, hh 0.5
BOX_B = np.array([30.0, 5.0, 0.0, 2.0, 4.0, 2.0, np.pi / 2])    # r = pi/2: u = dy, v = -dx (+ 6.1e-17 of the other); hl 1, hw 2, hh 1


def edge_points():
    """-> (cloud (N,4) float32, boxes [BOX_A, BOX_B], owner (N,), face (N,)): the expected values are written down here, not
    computed.  In box A every product is exact.  In box B the host's cos(pi/2) = 6.1e-17 is part of the rules: a point on
    the length axis has v = dy * 6.1e-17, far below every threshold used here; the one case where it decides is marked."""
    f32, nz = np.float32, np.float32(-0.0)
    up, dn = f32(np.inf), f32(-np.inf)
    rows = [
        # box A: the centre, -0.0 offsets (u = -0.0 is not < 0: face 0)
        ((0, 0, 0), 0, 0), ((nz, nz, nz), 0, 0), ((1, nz, 0), 0, 0), ((nz, 0.5, 0), 0, 2), ((0, nz, 0.25), 0, 4), ((nz, nz, -0.25), 0, 5),
        # the three diagonal ties go to the lower axis; the sign is that axis's
        ((1, 0.5, 0), 0, 0), ((-1, 0.5, 0), 0, 1), ((1, 0, 0.25), 0, 0), ((-1, 0, -0.25), 0, 1), ((0, 0.5, 0.25), 0, 2),
        ((0, -0.5, 0.25), 0, 3), ((1, 0.5, 0.25), 0, 0), ((-1, -0.5, -0.25), 0, 1),
        # just off the ties
        ((1, np.nextafter(f32(0.5), up), 0), 0, 2), ((0, 0.5, np.nextafter(f32(0.25), up)), 0, 4),
        # on each face (inclusive) and the float32 neighbour outside
        ((2, 0, 0), 0, 0), ((-2, 0, 0), 0, 1), ((0, 1, 0), 0, 2), ((0, -1, 0), 0, 3), ((0, 0, 0.5), 0, 4), ((0, 0, -0.5), 0, 5),
        ((np.nextafter(f32(2), up), 0, 0), -1, -1), ((np.nextafter(f32(-2), dn), 0, 0), -1, -1),
        ((0, np.nextafter(f32(1), up), 0), -1, -1), ((0, np.nextafter(f32(-1), dn), 0), -1, -1),
        ((0, 0, np.nextafter(f32(0.5), up)), -1, -1), ((0, 0, np.nextafter(f32(-0.5), dn)), -1, -1),
        # a corner: all three faces at once, a triple tie
        ((2, 1, 0.5), 0, 0), ((-2, -1, -0.5), 0, 1),
        # a NaN in each coordinate: no owner
        ((np.nan, 0, 0), -1, -1), ((0, np.nan, 0), -1, -1), ((0, 0, np.nan), -1, -1),
        # box B (centre 30, 5, 1): the centre; on each face and outside
        ((30, 5, 1), 1, 0), ((30, 6, 1), 1, 0), ((30, 4, 1), 1, 1), ((28, 5, 1), 1, 2), ((32, 5, 1), 1, 3), ((30, 5, 2), 1, 4), ((30, 5, 0), 1, 5),
        ((30, np.nextafter(f32(6), up), 1), -1, -1), ((30, np.nextafter(f32(4), dn), 1), -1, -1),
        ((np.nextafter(f32(28), dn), 5, 1), -1, -1), ((np.nextafter(f32(32), up), 5, 1), -1, -1),
        ((30, 5, np.nextafter(f32(2), up)), -1, -1), ((30, 5, np.nextafter(f32(0), dn)), -1, -1),
        # ties of box B that the small cosine does not touch: u = 0.5 exactly against w = 0.5; v = 1 against w = 0.5
        ((30, 5.5, 1.5), 1, 0), ((30, 4.5, 0.5), 1, 1), ((29, 5, 1.5), 1, 2), ((31, 5, 0.5), 1, 3),
        # and the one it decides: dx = -1, dy = 0.5 is a tie of |u| / hl and |v| / hw in exact arithmetic, but
        # u = -1 * 6.1e-17 + 0.5 rounds to the float64 below 0.5 while v = 1 + 0.5 * 6.1e-17 rounds to 1: axis 1
        ((29, 5.5, 1), 1, 2),
    ]
    cloud = np.array([list(p) + [0.25 + 0.001 * i] for i, (p, _, _) in enumerate(rows)], dtype=np.float32)
    return cloud, [BOX_A.copy(), BOX_B.copy()], np.array([o for _, o, _ in rows]), np.array([f for _, _, f in rows])


# ---------------------------------------------------------------------------------------------------------------------
# the dense random case: 8 non-overlapping boxes with 240 points each + 4001 background rows, shuffled
# ---------------------------------------------------------------------------------------------------------------------
def dense_case(seed):
    """-> (cloud (5921,4) float32, boxes (8,7)): boxes on a 4 x 2 grid of 12 m cells (each fits a circle of radius 3.2 m
    about its cell's centre whatever its yaw: they cannot overlap), 240 points uniform in each box shrunk by 1 %, 4001
    background rows over the whole area at z in [3, 5] — above every box —, one permutation of the rows"""
    rng = np.random.default_rng(seed)
    boxes, rows = [], []
    for k in range(8):
        l, w, h = rng.uniform(3.0, 5.0), rng.uniform(1.4, 2.2), rng.uniform(1.3, 2.0)
        b = np.array([10.0 + 12.0 * (k % 4), -6.0 + 12.0 * (k // 4), rng.uniform(-2.0, -1.0), h, w, l, rng.uniform(-np.pi, np.pi)])
        boxes.append(b)
        q = rng.uniform(-0.99, 0.99, (240, 3)) * np.array([l / 2, w / 2, h / 2])
        c, s = np.cos(b[6]), np.sin(b[6])
        rows.append(np.stack([b[0] + q[:, 0] * c - q[:, 1] * s, b[1] + q[:, 0] * s + q[:, 1] * c, b[2] + h / 2 + q[:, 2],
                              rng.uniform(0, 1, 240)], 1))
    rows.append(rng.uniform([0, -15, 3, 0], [60, 15, 5, 1], (4001, 4)))
    cloud = np.concatenate(rows).astype(np.float32)
    return np.ascontiguousarray(cloud[rng.permutation(len(cloud))]), np.array(boxes)


def dense_table(boxes, key0=0x9E3779B9):
    """the hand-made table of the dense case: every branch of the rules fires (asserted by the test on this restatement)
      0: pyramid 0 dropped; pyramid 0 also marked for thinning (drop wins); swaps pyramid 2 with entry 1
      1: pyramid 3 thinned (minimum 16: it applies); swaps pyramid 2 with entry 0
      2: pyramid 1 marked for thinning with a minimum of 64 (it does not apply: a pyramid holds ~40 points)
      3: swaps pyramid 4 with entry 5;  5: swaps pyramid 4 with entry 3 and has pyramid 4 dropped (drop wins over swap)
      4: swap_mask set but swap_with = -1;  6: swap_mask set and swap_with = 6, its own index;  7: nothing"""
    half = 1 << 23
    t = [entry(b) for b in boxes]
    t[0].update(drop_mask=1 << 0, sparse_mask=1 << 0, sparse_key=key0, sparse_thresh=half, sparse_min=16)
    t[1].update(sparse_mask=1 << 3, sparse_key=key0 + 1, sparse_thresh=half, sparse_min=16)
    t[2].update(sparse_mask=1 << 1, sparse_key=key0 + 2, sparse_thresh=half, sparse_min=64)
    pair(t, 0, 1, boxes, 2)
    pair(t, 3, 5, boxes, 4)
    t[5].update(drop_mask=1 << 4)
    t[4].update(swap_mask=0x3F, swap_with=-1)
    t[6].update(swap_mask=0x3F, swap_with=6)
    return t
