"""NumPy restatement of the composed augmentation (object noise -> flip -> rotation -> scaling -> translation:
voxelnet_amd/augment.py's draw_compose + csrc/augment.hip's vn_augment_compose) — the arbiter of the device kernel and of
the host draw.

Written on its own from the specification, sharing with the package only the primitives the specification names:
targets.label_to_gt_box_3d for the starting boxes, targets._limit_angle, augment.footprints_overlap (THE collision test of
the draw) and NumPy's cos / sin.
  - every float64 expression is elementwise and spelled exactly as the specification writes it (no matmul: a BLAS may
    fuse a multiply and an add), rounded once to float32;
  - membership is decided once, on the ORIGINAL cloud and the UNMOVED boxes, lowest table index first; a point takes at
    most one object move;
  - the draw keeps plain Python lists and dicts (no structured table).
A recipe is a dict with the keys of ComposeRecipe (`recipe()` gives the defaults)."""
import numpy as np

from voxelnet_amd.augment import footprints_overlap
from voxelnet_amd.targets import _limit_angle, label_to_gt_box_3d


def recipe(**kw):
    r = dict(object_rot=np.pi / 4, object_sigma=(1.0, 1.0, 0.5), attempts=100, flip=0.5, rotation=np.pi / 4,
             scale=(0.95, 1.05), translate_sigma=None)
    r.update(kw)
    return r


def entry(box, tx, ty, tz, rz):
    """table entry of an UNMOVED (7,) box (x, y, z, h, w, l, r) and its move: a dict of float64"""
    return dict(x=box[0], y=box[1], z0=box[2], z1=box[2] + box[3], hl=box[5] / 2, hw=box[4] / 2, c=np.cos(box[6]),
                s=np.sin(box[6]), tx=tx, ty=ty, tz=tz, rc=np.cos(rz), rs=np.sin(rz))


def affine(flip_y, angle, factor, translate):
    """stages 2-5 composed in that order, float64: (x, y) -> (x, fy*y) -> (X*c + Y*s, -(X*s) + Y*c) -> *f -> +t.  A stage
    that is off passes None."""
    fy = -1.0 if flip_y else 1.0
    c, s = (1.0, 0.0) if angle is None else (np.cos(angle), np.sin(angle))
    f = 1.0 if factor is None else float(np.float32(factor))
    t = (0.0, 0.0, 0.0) if translate is None else translate
    return dict(a00=f * c, a01=f * (s * fy), a10=f * (-s), a11=f * (c * fy), sz=f, bx=t[0], by=t[1], bz=t[2])


def draw(labels, rec):
    """the host draw from the global np.random state -> dict(before, after, has_box, table, lines, flip_y, angle, factor,
    translate, affine); table = entry() dicts of the accepted moves in label order, lines = their label-line indices"""
    boxes = label_to_gt_box_3d([labels], "", "lidar")[0].copy()
    before = boxes.copy()
    has_box = [line.split()[0] != "DontCare" for line in labels]
    real = [i for i, h in enumerate(has_box) if h]
    table, lines = [], []
    if rec["attempts"] and not (rec["object_rot"] is None and rec["object_sigma"] is None):
        rot = rec["object_rot"] if rec["object_rot"] is not None else 0.0
        sig = rec["object_sigma"] if rec["object_sigma"] is not None else (0.0, 0.0, 0.0)
        for i in real:
            for _attempt in range(rec["attempts"]):
                rz = np.random.uniform(-rot, rot)
                tx = np.random.normal() * sig[0]
                ty = np.random.normal() * sig[1]
                tz = np.random.normal() * sig[2]
                b = boxes[i]
                cand = np.array([b[0] + tx, b[1] + ty, b[2] + tz, b[3], b[4], b[5], _limit_angle(b[6] + rz)])
                if any(footprints_overlap(cand, boxes[j]) for j in real if j != i):
                    continue
                table.append(entry(before[i], tx, ty, tz, rz))
                lines.append(i)
                boxes[i] = cand
                break
    flip_y, angle, factor, translate = False, None, None, None
    if rec["flip"]:
        flip_y = bool(np.random.random() < rec["flip"])
        if flip_y:
            for i in real:
                boxes[i, 1] = -boxes[i, 1]
                boxes[i, 6] = -boxes[i, 6]
    if rec["rotation"] is not None:
        angle = float(np.random.uniform(-rec["rotation"], rec["rotation"]))
        c, s = np.cos(angle), np.sin(angle)
        for i in real:
            X, Y = boxes[i, 0], boxes[i, 1]
            boxes[i, 0] = X * c + Y * s
            boxes[i, 1] = -(X * s) + Y * c
            boxes[i, 6] = boxes[i, 6] - angle
    if rec["scale"] is not None:
        factor = float(np.random.uniform(rec["scale"][0], rec["scale"][1]))
        for i in real:
            boxes[i, 0:6] *= factor
    if rec["translate_sigma"] is not None:
        translate = tuple(float(np.random.normal() * sg) for sg in rec["translate_sigma"])
        for i in real:
            boxes[i, 0] += translate[0]
            boxes[i, 1] += translate[1]
            boxes[i, 2] += translate[2]
    return dict(before=before, after=boxes, has_box=np.array(has_box, dtype=bool), table=table, lines=lines, flip_y=flip_y,
                angle=angle, factor=factor, translate=translate, affine=affine(flip_y, angle, factor, translate))


def inside(cloud, e):
    """(N,) bool: the original float32 points, widened exactly, inside entry e's unmoved box (inclusive; NaN fails)"""
    px, py, pz = (cloud[:, a].astype(np.float64) for a in range(3))
    with np.errstate(invalid="ignore"):
        dx, dy = px - e["x"], py - e["y"]
        u = dx * e["c"] + dy * e["s"]
        v = -(dx * e["s"]) + dy * e["c"]
        return (np.abs(u) <= e["hl"]) & (np.abs(v) <= e["hw"]) & (pz >= e["z0"]) & (pz <= e["z1"])


def owner(cloud, table):
    """(N,) int: the lowest table index whose unmoved box holds the original point, else -1"""
    own = np.full(len(cloud), -1, dtype=np.int64)
    for b in range(len(table) - 1, -1, -1):
        own[inside(cloud, table[b])] = b
    return own


def apply(cloud, table, aff):
    """cloud (N,4) float32 -> the augmented copy; table: entry() dicts, aff: an affine() dict"""
    cloud = np.asarray(cloud, dtype=np.float32)
    px, py, pz = (cloud[:, a].astype(np.float64) for a in range(3))
    X, Y, Z = px.copy(), py.copy(), pz.copy()
    own = owner(cloud, table)
    for b, e in enumerate(table):
        m = own == b
        dx, dy = px[m] - e["x"], py[m] - e["y"]
        X[m] = (e["x"] + e["tx"]) + (dx * e["rc"] - dy * e["rs"])
        Y[m] = (e["y"] + e["ty"]) + (dx * e["rs"] + dy * e["rc"])
        Z[m] = pz[m] + e["tz"]
    out = cloud.copy()
    with np.errstate(invalid="ignore"):
        out[:, 0] = ((aff["a00"] * X + aff["a01"] * Y) + aff["bx"]).astype(np.float32)
        out[:, 1] = ((aff["a10"] * X + aff["a11"] * Y) + aff["by"]).astype(np.float32)
        out[:, 2] = (aff["sz"] * Z + aff["bz"]).astype(np.float32)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# bridges to the package's types (tests only)
# ---------------------------------------------------------------------------------------------------------------------
FIELDS = ("x", "y", "z0", "z1", "hl", "hw", "c", "s", "tx", "ty", "tz", "rc", "rs")
AFFINE = ("a00", "a01", "a10", "a11", "sz", "bx", "by", "bz")


def to_params(table, aff):
    """entry() dicts + an affine() dict -> the package's ComposeParams (no boxes: for the device wrappers only)"""
    from voxelnet_amd import augment as A
    t = np.zeros(len(table), dtype=A.MOVE_DTYPE)
    for i, e in enumerate(table):
        for n in FIELDS:
            t[i][n] = e[n]
    z = np.zeros((0, 7))
    return A.ComposeParams(z, z, np.zeros(0, dtype=bool), t, [], False, 0.0, 1.0, (0.0, 0.0, 0.0),
                           np.array([aff[n] for n in AFFINE], dtype=np.float64))


def same_draw(p, d):
    """the package's ComposeParams equals the restatement's draw, field by field, bit for bit"""
    ok = p.boxes_before.tobytes() == d["before"].tobytes() and p.boxes_after.tobytes() == d["after"].tobytes()
    ok = ok and np.array_equal(p.has_box, d["has_box"]) and list(p.entry_line) == d["lines"] and len(p.table) == len(d["table"])
    ok = ok and all(float(row[n]) == float(e[n]) for row, e in zip(p.table, d["table"]) for n in FIELDS)
    ok = ok and p.flip_y == d["flip_y"] and p.angle == (d["angle"] or 0.0) and p.factor == (1.0 if d["factor"] is None else d["factor"])
    ok = ok and tuple(p.translate) == (d["translate"] or (0.0, 0.0, 0.0))
    return ok and np.array([d["affine"][n] for n in AFFINE]).tobytes() == np.asarray(p.affine, dtype=np.float64).tobytes()


def frame(f, per_car=40):
    """the frames of the compose tests: a 6,000-point cloud with six cars that HOLD points.  The generator's cloud is
    uniform over the crop — a car-sized box holds 3..10 of 6,000 points, too few for a test that wants every moved object
    to carry at least 20 — so each car gets `per_car` points of its own, uniform inside its box shrunk by 2 % (clear of
    the faces), in front of the first 6000 - 6 * per_car rows of synth.synth_cloud("Car", 6000, frame_seed(2, f), 2.3, 35)
    (the generator's output is already permuted: a prefix is a uniform subsample); then one permutation.
    -> (cloud (6000,4) float32 without exact zeros, label lines: six cars + one DontCare)"""
    from voxelnet_amd import synth
    base = synth.synth_cloud("Car", 6000, synth.frame_seed(2, f), 2.3, 35)
    labels = synth.synth_labels("Car", 6, f)
    boxes = label_to_gt_box_3d([labels], "", "lidar")[0][:6]
    rng = np.random.default_rng(7000 + f)
    own = []
    for b in boxes:
        u = rng.uniform(-0.98, 0.98, (per_car, 2)) * np.array([b[5] / 2, b[4] / 2])
        c, s = np.cos(b[6]), np.sin(b[6])
        own.append(np.stack([b[0] + u[:, 0] * c - u[:, 1] * s, b[1] + u[:, 0] * s + u[:, 1] * c,
                             b[2] + rng.uniform(0.01, 0.99, per_car) * b[3], np.round(rng.uniform(0, 1, per_car), 2)], 1))
    cloud = np.concatenate(own + [base[:6000 - 6 * per_car]]).astype(np.float32)
    cloud = cloud[rng.permutation(len(cloud))]
    cloud[:, :3][cloud[:, :3] == 0] = np.float32(1e-3)
    return np.ascontiguousarray(cloud), labels
